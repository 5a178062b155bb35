"""Trajectories on the MI355X (csrc/ngw_traj.inc, the TRAJ forms of ngw_slot_rollout_kernel / ngw_playout_kernel, include/ngw.h
ngw_snapshot_rollout_traj / ngw_snapshot_playout_traj), held to the CPU oracle (tests/trajectory_oracle.py: the oracle's steps on a host copy of the
parents' rows, its masks on the row before every step, its lidar on the parent and on every visited row - never the device's own step, mask or
lidar).  Everything is an integer and compared bit for bit.

Inputs.  A random playout of nine steps does not reach the goal, so a configuration without deaths would never end a pair and neither the zero
rows nor an episode's last row would be tested.  Every configuration but the plain fire10h therefore runs under autoreset with a horizon of 6 and
the envs' step counters are set to env % 6 after the warm-up (on the oracle and on the device alike): parent e is cut after 6 - e % 6 steps, so
every shape with T = 5 holds pairs that end before T and pairs that run all T steps.  The plain fire10h ends pairs by deaths.  The oracle side of
these conditions needs no GPU and was checked on the CPU when the seeds were chosen; every test asserts them again."""
import functools
import re

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import path_key_oracle as KO
import playout_oracle as PO
import sample_oracle as SO
import slot_observe_oracle as OO
import slot_rollout_oracle as RO
import trajectory_oracle as TO
from gym_novel_gridworlds_amd import LimitActions, VecNovelGridworld
from gym_novel_gridworlds_amd.playout import Playout, PlayoutPath, PlayoutTraj, choose_actions
from gym_novel_gridworlds_amd.snapshot import MapsTooLarge, transitions
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from gym_novel_gridworlds_amd.vec_env import PlanEval, RolloutPath, RolloutTraj
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
STATE_KEYS = PO.STATE_KEYS
SEED = 0x5EED0123456789AB
N = 20
HORIZON = 6
SHAPES = ((1, 1), (65, 5), (200, 9))                            # (pairs, T): a lone lane / one past a wave / a ragged last wave
FORMATS = {'int32': np.int32, 'int16': np.int16, 'packed': 'packed'}
# configuration, autoreset with a horizon of 6, the lidar row format, the event the oracle must see inside the paths (None: none beyond the ends)
CONFIGS = [('pogo10', True, 'int32', None), ('pogo10', True, 'int16', None), ('pogo10', True, 'packed', None), ('pogo13', True, 'int16', None),
           ('axe10', True, 'packed', 'pickups'), ('fire10h', False, 'int32', 'deaths'), ('fire10h', True, 'int16', 'cuts'), ('crate11e', True, 'int32', 'inv_jumps'),
           ('add32', True, 'packed', None)]


@functools.lru_cache(maxsize=None)
def twin(cfg, auto, n=N, warm=10, beams=8):
    """The oracle after `warm` random steps with its step counters spread over the horizon, and what a device env needs to be its twin."""
    spec = T.build_spec(cfg)
    seed = XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=HORIZON) if auto else {}
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    o.reset()
    rs = np.random.RandomState(n + warm)
    warmup = [rs.randint(0, len(spec.actions_id), n).astype(np.int32) for _ in range(warm)]
    for a in warmup:
        o.step(a)
    if auto:
        o.st.step_count[...] = np.arange(n) % HORIZON
    return spec, o, seed, kw, warmup, OO.lidar_config(cfg, beams)


def make(cfg, auto, fmt='int32', n=N, beams=8):
    spec, o, seed, kw, warmup, lc = twin(cfg, auto, n, beams=beams)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    v.reset()
    for a in warmup:
        v.step(a)
    if auto:
        v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    v.lidar_configure(lc, dtype=FORMATS[fmt])
    return spec, v, o, lc


def case_inputs(spec, n, count, steps, salt=0):
    """The parents (with repeats), the plans [count, T] and the weights of one shape: a function of the shape alone."""
    rs = np.random.RandomState(1000 * salt + 7 * count + steps)
    A = len(spec.actions_id)
    return rs.randint(0, n, count), rs.randint(0, A, (count, steps)), SO.random_weights(rs, 1, A)[0]


@functools.lru_cache(maxsize=None)
def expected(cfg, auto, count, steps, salt=0, beams=8):
    """The oracle's side of one shape for the three calls, computed once and shared (nobody writes to it)
    -> (parents, plans, weights, {kind: oracle_traj's dict with 'actions' [T, count]})."""
    spec, o, _, _, _, lc = twin(cfg, auto, beams=beams)
    parents, plans, x = case_inputs(spec, N, count, steps, salt)
    hz = HORIZON if auto else 0
    _, _, acts_u, _ = PO.oracle_playout(spec, o.st, parents, steps, SEED, 0, auto, hz)
    _, _, acts_w, _ = SO.oracle_weighted_playout(spec, o.st, parents, steps, SEED, x, 0, auto, hz)
    out = {}
    for kind, acts in (('playout', acts_u), ('weighted', acts_w), ('rollout', plans.T)):
        out[kind] = TO.oracle_traj(spec, o.st, parents, acts, None, auto, hz, lc=lc)
        out[kind]['actions'] = acts
    return parents, plans, x, out


def input_conditions(cfg, auto, event):
    """What the oracle's paths must contain for the tests to be about anything (needs no GPU) -> the counts, for the record."""
    short = full = seen = 0
    rows = np.zeros(3, np.int64)                                    # non-zero rows, executed steps, non-zero last rows of pairs that end early
    for count, steps in SHAPES:
        for e in expected(cfg, auto, count, steps)[3].values():
            rep = e['reports']
            short += int((rep['ended'] & (rep['length'] < steps)).sum())
            full += int((rep['length'] == steps).sum())
            seen += e['events'][event] if event else 1
            assert ((e['keys'] != 0).sum(0) == rep['length']).all() and ((e['masks'] != 0).sum(0) == rep['length']).all()
            shown = e['obs'][1:].any(2)                             # (an agent that sees nothing and holds nothing observes zeros: most do not)
            early = np.nonzero((rep['length'] < steps) & (rep['length'] > 0))[0]
            rows += np.array([shown.sum(), rep['length'].sum(), shown[rep['length'][early] - 1, early].sum()])
        if steps == 5:
            e = expected(cfg, auto, count, steps)[3]['playout']['reports']
            assert (e['ended'] & (e['length'] < steps)).any() and (e['length'] == steps).any(), (cfg, auto, 'the T = 5 playouts need both a short and a full pair')
    assert short > 0 and full > 0, "%s auto=%d: %d pairs end before T, %d run all T steps: neither the zero rows nor the last row is tested" % (cfg, auto, short, full)
    assert 2 * rows[0] > rows[1] and rows[2] > 0, "too few non-zero rows (%d of %d, %d last ones): the zero rows behind an end would prove nothing" % tuple(rows)
    assert seen > 0, "%s: the oracle met no '%s' inside the paths: the inputs are wrong" % (cfg, event)
    return short, full, seen


def assert_result(got, e, where, kids_rows=None):
    if hasattr(got.ret, 'data_ptr'):                                # a result on the device: the same bits on the host
        got = type(got)(*[None if x is None else OO.host(x) for x in got])._replace(info=OO.host(got.info).view(np.uint32))
    RO.assert_reports(got, e['reports'], where)
    if getattr(got, 'actions', None) is not None:
        assert (OO.host(got.actions) == e['actions']).all(), where
    TO.assert_traj(got, e, where, [k for k in ('rewards', 'masks', 'obs') if getattr(got, k, None) is not None])
    if got.keys is not None:
        KO.assert_keys(got.keys, e['keys'], where)
    assert (OO.host(got.rewards).sum(0) == OO.host(got.ret)).all(), where
    if kids_rows is not None:
        RO.assert_rows(kids_rows[0].state(), e['ends'], where, idx=kids_rows[1])


@pytest.mark.parametrize('cfg,auto,fmt,event', CONFIGS)
def test_against_the_oracle(cfg, auto, fmt, event):
    """Rollout, playout and weighted playout at every shape, every field asked for together, from the same pool with repeated parents, from the
    envs and from another pool (the three hold the same rows, so one oracle run serves them)."""
    input_conditions(cfg, auto, event)
    spec, v, o, lc = make(cfg, auto, fmt)
    n, cap = v.num_envs, 512
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    for count, steps in SHAPES:
        parents, plans, x, exp = expected(cfg, auto, count, steps)
        kids = n + np.random.RandomState(count).permutation(cap - n)[:count] if steps == 5 else None
        for src, kw in (('same pool', {}), ('from the envs', dict(from_envs=True)), ('another pool', dict(source=other))):
            where = '%s auto=%d %s count=%d T=%d %s' % (cfg, auto, fmt, count, steps, src)
            keyed = src == 'same pool'
            for kind in ('playout', 'weighted'):
                p = pool.playout(parents, steps, SEED, kids, record=True, rewards=True, masks=True, observe='lidar', path_keys=keyed,
                                 weights=x if kind == 'weighted' else None, **kw)
                assert isinstance(p, PlayoutTraj) and (p.keys is not None) == keyed
                row = p.obs[0] if fmt == 'packed' else p.obs
                assert row.dtype == (np.uint8 if fmt == 'packed' else FORMATS[fmt]) and row.shape[:2] == (steps + 1, count)
                assert_result(p, exp[kind], where + ' ' + kind, None if kids is None else (pool, kids))
            r = pool.rollout(parents, plans, kids, rewards=True, observe='lidar', path_keys=keyed, **kw)
            assert isinstance(r, RolloutTraj) and (r.keys is not None) == keyed
            assert_result(r, exp['rollout'], where + ' rollout', None if kids is None else (pool, kids))
    # the rows are the rows the slot observation returns: same dtype, same layout
    one = pool.lidar_observation(np.arange(n))
    p = pool.playout(np.arange(n), 1, SEED, observe='lidar')
    for a, b in zip(one if fmt == 'packed' else (one,), p.obs if fmt == 'packed' else (p.obs,)):
        assert a.dtype == b.dtype and a.shape == b.shape[1:] and (a == b[0]).all()
    assert p.rewards is None and p.masks is None and p.keys is None
    assert v.error_flags() == 0
    v.close()


# a beam count that is no multiple of 4 has no world-frame table (ngw_lidar_configure): the rows are marched through the 8 KiB per-lane ray table, which
# the TRAJ forms stage ONCE in front of the T-loop; 8 beams never touch it.  Odd and even row lengths, the smallest and the largest map class.
@pytest.mark.parametrize('cfg,fmt,beams', [('pogo13', 'int16', 10), ('pogo10', 'packed', 10), ('add32', 'int32', 7)])
def test_the_per_lane_ray_table_form_against_the_oracle(cfg, fmt, beams):
    """Playout, weighted playout and rollout with T > 1, every field with keys, rows marched through the staged ray table: the table must survive
    every step of the loop (a table clobbered by the steps, the tile or the shadows would show from obs[1] on, one staged wrong from obs[0] on)."""
    spec, v, o, lc = make(cfg, True, fmt, beams=beams)
    assert lc.num_beams % 4 != 0
    n = v.num_envs
    pool = v.snapshot(n + 256)
    pool.save(slots=np.arange(n))
    late = 0
    for count, steps in SHAPES[1:]:
        parents, plans, x, exp = expected(cfg, True, count, steps, beams=beams)
        kids = n + np.arange(count)
        for keyed in (True, False):
            where = '%s %s %d beams count=%d T=%d keys=%d' % (cfg, fmt, beams, count, steps, keyed)
            for kind in ('playout', 'weighted'):
                p = pool.playout(parents, steps, SEED, kids, record=True, rewards=True, masks=True, observe='lidar', path_keys=keyed,
                                 weights=x if kind == 'weighted' else None)
                assert_result(p, exp[kind], where + ' ' + kind, (pool, kids))
            r = pool.rollout(parents, plans, kids, rewards=True, observe='lidar', path_keys=keyed)
            assert_result(r, exp['rollout'], where + ' rollout', (pool, kids))
        late += sum(int(e['obs'][3:].any(2).sum()) for e in exp.values())
        # ... and the rows are the slot observation's, which stages the table per call
        one = pool.lidar_observation(kids)
        last = TO.widen(r.obs)[r.length, np.arange(count)]
        assert (TO.widen(one) == last).all() and (last == exp['rollout']['obs'][exp['rollout']['reports']['length'], np.arange(count)]).all()
    assert late > 100, "too few non-zero rows behind the second step: a table lost inside the loop would not show"
    assert v.error_flags() == 0
    v.close()


def test_the_recorded_words_reproduce_the_recorded_actions():
    from gym_novel_gridworlds_amd.playout import playout_words
    from gym_novel_gridworlds_amd.sample import choose_weighted
    spec, v, o, lc = make('crate11e', True)
    pool = v.snapshot(N)
    pool.save()
    count, steps, A = 200, 9, v.n_actions
    parents, _, x, exp = expected('crate11e', True, count, steps)
    pairs = 7 + np.arange(count, dtype=np.uint64)
    p = pool.playout(parents, steps, SEED, record=True, masks=True, first_pair=7)
    w = pool.playout(parents, steps, SEED, record=True, masks=True, first_pair=7, weights=x)
    assert p.rewards is None and p.obs is None and p.masks.dtype == np.uint64
    for t in range(steps):
        ran = p.length > t
        assert (choose_actions(p.masks[t][ran], SEED, pairs[ran], t, A) == p.actions[t][ran]).all() and (p.masks[t][~ran] == 0).all()
        ran = w.length > t
        got = choose_weighted(w.masks[t][ran], np.broadcast_to(x, (int(ran.sum()), A)), SEED, pairs[ran], t, A, words=playout_words(SEED, pairs[ran], t))
        assert (np.asarray(got[0]) == w.actions[t][ran]).all() and (w.masks[t][~ran] == 0).all()
    v.close()


def test_limits_give_the_prefix_and_first_pair_splits_give_the_whole():
    import torch
    spec, v, o, lc = make('fire10h', True, 'int16')
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n)
    pool.save()
    parents, plans, x, exp = expected('fire10h', True, count, steps)
    rs = np.random.RandomState(4)
    limits = rs.randint(0, steps + 1, count)
    limits[:4] = [0, steps, 0, 1]
    cut = np.arange(steps)[:, None] >= limits[None, :]
    cut_rows = np.arange(steps + 1)[:, None] > limits[None, :]
    for kind, call in (('playout', lambda **k: pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, observe='lidar', path_keys=True, **k)),
                       ('weighted', lambda **k: pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, observe='lidar', weights=x, **k)),
                       ('rollout', lambda **k: pool.rollout(parents, plans, rewards=True, observe='lidar', path_keys=True, **k))):
        whole, part = call(), call(limits=limits)
        assert_result(whole, exp[kind], kind)
        e = TO.oracle_traj(spec, o.st, parents, exp[kind]['actions'], limits, True, HORIZON, lc=lc)
        e['actions'] = np.where(cut, -1, exp[kind]['actions'])
        assert e['events']['limited'] > 0
        assert_result(part, e, 'limited ' + kind)
        assert (part.rewards == np.where(cut, 0, whole.rewards)).all() and (part.obs == np.where(cut_rows[:, :, None], 0, whole.obs)).all()
        if kind != 'rollout':
            assert (part.masks == np.where(cut, np.uint64(0), whole.masks)).all()
        # obs[limit] is the last non-zero row of a pair its limit cut
        shorter = np.nonzero(limits < whole.length)[0]
        seen = [j for j in shorter if whole.obs[limits[j], j].any()]
        assert len(seen) > len(shorter) // 2 and all(part.obs[limits[j], j].any() and not part.obs[limits[j] + 1:, j].any() for j in seen)
        assert (part.obs[0] == whole.obs[0]).all() and part.obs[0, limits == 0].any()               # a limit of 0 still observes the parent
        # two halves with first_pair set: the whole call
        if kind != 'rollout':
            h = 70
            kw = dict(weights=x) if kind == 'weighted' else dict(path_keys=True)
            lo = pool.playout(parents[:h], steps, SEED, record=True, rewards=True, masks=True, observe='lidar', **kw)
            hi = pool.playout(parents[h:], steps, SEED, record=True, rewards=True, masks=True, observe='lidar', first_pair=h, **kw)
            for name in ('actions', 'rewards', 'masks', 'obs') + (('keys',) if kind == 'playout' else ()):
                assert (np.concatenate([lo[name], hi[name]], 1) == whole[name]).all(), (kind, name)
    # path keys with observations are the plain path call's keys
    plain = pool.playout(parents, steps, SEED, path_keys=True)
    assert type(plain) is PlayoutPath and (plain.keys == exp['playout']['keys']).all()
    # on the device: the fields stay there, in torch's types, ordered behind the launch
    d = pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, observe='lidar', device=True)
    assert d.rewards.dtype == torch.int32 and d.masks.dtype == torch.int64 and d.obs.dtype == torch.int16 and d.obs.is_cuda and tuple(d.obs.shape[:2]) == (steps + 1, count)
    assert_result(d, exp['playout'], 'device')
    t, j = transitions(d)
    assert int(t.numel()) == int(exp['playout']['reports']['length'].sum()) and (d.obs[t + 1, j].cpu().numpy() == exp['playout']['obs'][t.cpu().numpy() + 1, j.cpu().numpy()]).all()
    assert v.error_flags() == 0
    v.close()


def test_device_cross_check_a_limited_replay_observes_the_recorded_row():
    """obs[t + 1, j] equals snap.lidar_observation of the child a rollout of pair j's recorded actions leaves with limits = t + 1."""
    spec, v, o, lc = make('axe10', True, 'packed')
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n + 64)
    pool.save(slots=np.arange(n))
    parents = np.random.RandomState(1).randint(0, n, count)
    play = pool.playout(parents, steps, SEED, record=True, observe='lidar', rewards=True)
    ts, js = transitions(play)
    pick = np.random.RandomState(2).permutation(len(ts))[:12]
    pick = np.concatenate([pick, [np.argmax(ts)]])                   # (a last step among them)
    ts, js = ts[pick], js[pick]
    kids = n + np.arange(len(pick))
    r = pool.rollout(parents[js], np.maximum(play.actions[:, js].T, 0), kids, limits=ts + 1, rewards=True)   # (-1 behind an end: beyond the limit)
    assert isinstance(r, RolloutTraj) and (r.length == ts + 1).all() and (r.rewards[ts, np.arange(len(ts))] == play.rewards[ts, js]).all()
    beams, inv = pool.lidar_observation(kids)
    assert (beams == play.obs[0][ts + 1, js]).all() and (inv == play.obs[1][ts + 1, js]).all() and beams.any(1).all()
    assert v.error_flags() == 0
    v.close()


def test_a_bad_parent_gives_zero_rows_and_columns_and_its_neighbours_are_unaffected():
    import torch
    spec, v, o, lc = make('axe10', True)
    n, count, steps = v.num_envs, 66, 5
    pool = v.snapshot(n)
    pool.save()
    parents, plans, _ = case_inputs(spec, n, count, steps, salt=5)
    good = np.ones(count, bool)
    good[[5, 64]] = False
    bad = parents.copy()
    bad[5], bad[64] = n, -1
    dev = torch.from_numpy(bad.astype(np.int32)).cuda()
    acts = torch.from_numpy(np.ascontiguousarray(plans.T.astype(np.int32))).cuda()
    torch.cuda.synchronize()
    p = pool.playout(dev, steps, SEED, record=True, rewards=True, masks=True, observe='lidar')
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    r = pool.rollout(dev, acts, rewards=True, observe='lidar')
    assert v.error_flags() == F_BAD_INDEX
    # the pairs around the bad lanes: each pair's stream is its position, so the good ones are what the oracle gives for them alone
    ends, rep, au, _ = PO.oracle_playout(spec, o.st, parents, steps, SEED, 0, True, HORIZON)
    eu = TO.oracle_traj(spec, o.st, parents, au, None, True, HORIZON, lc=lc)
    er = TO.oracle_traj(spec, o.st, parents, plans.T, None, True, HORIZON, lc=lc)
    for res, e, names in ((p, eu, ('rewards', 'masks', 'obs')), (r, er, ('rewards', 'obs'))):
        for name in names:
            assert (res[name][:, good] == e[name][:, good]).all(), name
            assert not res[name][:, ~good].any(), name                # obs[0] included
        for k in ('ret', 'length', 'ended', 'info'):
            assert (res[k][good] == e['reports'][k][good]).all() and (res[k][~good] == 0).all(), k
    assert (p.actions[:, ~good] == -1).all() and (p.actions[:, good] == au[:, good]).all()
    v.close()


def test_nothing_is_committed():
    spec, v, o, lc = make('fire10h', True, 'int16')
    n = v.num_envs
    pool = v.snapshot(n + 8)
    pool.save(slots=np.arange(n))
    v.action_masks(); v.lookahead()
    env_obs = v.lidar_observation(copy=True)

    def everything():
        st, la = v.get_state(), v.lookahead(copy=True)
        return ([np.asarray(st[k]).copy() for k in sorted(st)] + [np.asarray(x).copy() for x in la] + [v.action_mask_words().copy()] +
                [np.asarray(x).copy() for x in (pool.state()[k] for k in STATE_KEYS)])
    before = everything()
    parents, plans, x, _ = expected('fire10h', True, 200, 9)
    pool.playout(parents, 9, SEED, rewards=True, masks=True, observe='lidar', path_keys=True)
    pool.playout(parents, 9, SEED, rewards=True, masks=True, observe='lidar', from_envs=True, weights=x)
    pool.rollout(parents, plans, rewards=True, observe='lidar', from_envs=True)
    v.playouts(3, 5, SEED, rewards=True, masks=True, observe='lidar')
    after = everything()
    assert len(before) == len(after) and all((a == b).all() for a, b in zip(before, after))
    assert (v.lidar_observation() == env_obs).all()                 # the env's own lidar rows are its own
    assert v.error_flags() == 0
    v.close()


def test_plain_calls_are_unchanged():
    spec, v, o, lc = make('axe10', True)
    n = v.num_envs
    pool = v.snapshot(n)
    pool.save()
    parents, plans, x, exp = expected('axe10', True, 200, 9)
    a, b = pool.rollout(parents, plans), pool.rollout(parents, plans, rewards=False, masks=False, observe=None)
    assert type(a) is type(b) is PlanEval and all((p == q).all() for p, q in zip(a, b))
    RO.assert_reports(a, exp['rollout']['reports'], 'plain rollout')
    k = pool.rollout(parents, plans, path_keys=True, rewards=False)
    assert type(k) is RolloutPath
    KO.assert_keys(k.keys, exp['rollout']['keys'], 'path rollout')
    a, b = pool.playout(parents, 9, SEED, record=True), pool.playout(parents, 9, SEED, record=True, rewards=False, masks=False, observe=None)
    assert type(a) is type(b) is Playout and all((p == q).all() for p, q in zip(a, b))
    RO.assert_reports(a, exp['playout']['reports'], 'plain playout')
    assert (a.actions == exp['playout']['actions']).all()
    c = pool.playout(parents, 9, SEED, record=True, path_keys=True)
    assert type(c) is PlayoutPath and all((p == q).all() for p, q in zip(a, c[:6]))
    KO.assert_keys(c.keys, exp['playout']['keys'], 'path playout')
    d = pool.playout(parents, 9, SEED, record=True, rewards=True, masks=True, observe='lidar')
    assert all((p == q).all() for p, q in zip(a, d[:6]))             # the recording changes nothing else
    v.close()


def test_other_surfaces():
    """venv.playouts [T, N, P] / [T + 1, N, P, row], the single-env adapter [T, P] / [T + 1, P, row] and LimitActions in its own id space."""
    spec, v, o, lc = make('pogo10', True, n=3)
    P, steps = 2, 3
    par = np.repeat(np.arange(3), P)
    _, rep, acts, _ = PO.oracle_playout(spec, o.st, par, steps, SEED, 0, True, HORIZON)
    e = TO.oracle_traj(spec, o.st, par, acts, None, True, HORIZON, lc=lc)
    got = v.playouts(P, steps, SEED, rewards=True, masks=True, observe='lidar')
    assert isinstance(got, PlayoutTraj) and got.rewards.shape == (steps, 3, P) and got.masks.shape == (steps, 3, P) and got.obs.shape == (steps + 1, 3, P, e['obs'].shape[-1])
    assert got.actions is None and got.keys is None
    for name in ('rewards', 'masks', 'obs'):
        TO.assert_field(got[name].reshape((got[name].shape[0], 3 * P) + got[name].shape[3:]), e[name], 'venv.playouts', name)
    assert (got.length.reshape(-1) == rep['length']).all()
    v.close()
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    vec = env.unwrapped._backend()
    vec.lidar_configure(OO.lidar_config('axe10'), dtype=np.int16)
    rows = vec.get_state()
    P, steps = 5, 3
    lim = LimitActions(env, {'Break', 'Forward', 'Left'})
    for who in (env, lim):
        play = who.playouts(P, steps, SEED, rewards=True, masks=True, observe='lidar')
        sp = vec.spec if who is env else who.__dict__['_playout_env'][2].spec
        _, _, acts, _ = PO.oracle_playout(sp, rows, np.zeros(P, np.int64), steps, SEED)
        e = TO.oracle_traj(sp, rows, np.zeros(P, np.int64), acts, lc=vec.lidar)
        assert isinstance(play, PlayoutTraj) and play.rewards.shape == (steps, P) and play.obs.shape == (steps + 1, P, e['obs'].shape[-1]) and play.obs.dtype == np.int16
        TO.assert_traj(play, e, type(who).__name__, ('rewards', 'obs'))
        if who is env:
            TO.assert_field(play.masks, e['masks'], 'adapter', 'masks')
        else:                                                          # the words in the wrapper's ids, consistent with the actions it reports
            ids = [lim.limited_actions_id[name] for name in sorted(lim.limited_actions)]
            exp_words = sum(((e['masks'] >> np.uint64(i)) & np.uint64(1)) << np.uint64(j) for i, j in enumerate(ids))
            assert (play.masks == exp_words).all() and ((play.masks[0] >> play.first_action.astype(np.uint64)) & np.uint64(1)).all()
    lim.close()


def test_maps_the_layout_cannot_hold_are_refused_with_the_bytes():
    """47 x 47 (the largest map a lidar's range allows) fits the path form but not the observing form: the stand-alone lidar launch's layout needs
    166 160 B there.  lidar_configure says so (MapsTooLarge, naming the bytes), observe='lidar' is refused with the same bytes, and the same env
    still serves rewards and masks alone.  46 x 46 serves everything."""
    n = 4
    big = VecNovelGridworld(spec=make_spec(T.POGO, 47), num_envs=n, seed=4)
    big.reset()
    with pytest.raises(MapsTooLarge, match='needs 166160 B of LDS'):
        big.lidar_configure(num_beams=8, dtype=np.int32)
    assert big.lidar is None
    bs = big.snapshot(n)
    bs.save()
    for call in (lambda: bs.playout(np.arange(n), 3, SEED, observe='lidar'),
                 lambda: bs.rollout(None, np.zeros((n, 3), np.int64), from_envs=True, observe='lidar', rewards=True),
                 lambda: bs.playout(np.arange(n), 3, SEED, observe='lidar', path_keys=True),
                 lambda: big.playouts(2, 3, SEED, observe='lidar')):
        with pytest.raises(MapsTooLarge, match='map_size 47') as ex:
            call()
        need = re.search(r'needs (\d+) B of LDS \(> 160 KiB\)', str(ex.value))
        assert need and int(need.group(1)) == 166160, str(ex.value)
    r = bs.playout(np.arange(n), 3, SEED, rewards=True, masks=True, path_keys=True)
    assert isinstance(r, PlayoutTraj) and (r.rewards.sum(0) == r.ret).all() and (r.masks[0] != 0).all() and r.obs is None
    q = bs.rollout(None, np.zeros((n, 3), np.int64), from_envs=True, rewards=True)
    assert (q.rewards.sum(0) == q.ret).all()
    assert big.error_flags() == 0
    big.close()
    ok = VecNovelGridworld(spec=make_spec(T.POGO, 46), num_envs=n, seed=4)
    ok.reset()
    ok.lidar_configure(num_beams=8, dtype=np.int32)
    s = ok.snapshot(n)
    s.save()
    p = s.playout(np.arange(n), 3, SEED, observe='lidar', path_keys=True, rewards=True)
    assert (p.obs[0] == s.lidar_observation()).all() and (p.rewards.sum(0) == p.ret).all()
    # the per-lane ray table (a beam count that is no multiple of 4) takes 8 KiB more: 44 x 44 is served, with keys too; 45 x 45 is not
    t44 = VecNovelGridworld(spec=make_spec(T.POGO, 44), num_envs=n, seed=4)
    t44.reset()
    t44.lidar_configure(num_beams=10, dtype=np.int32)
    s = t44.snapshot(n)
    s.save()
    p = s.playout(np.arange(n), 3, SEED, observe='lidar', path_keys=True, rewards=True)
    r = s.rollout(np.arange(n), np.zeros((n, 3), np.int64), observe='lidar', path_keys=True)
    assert (p.obs[0] == s.lidar_observation()).all() and (r.obs[0] == p.obs[0]).all() and p.obs[0].any() and (p.rewards.sum(0) == p.ret).all()
    assert t44.error_flags() == 0
    t44.close()
    t45 = VecNovelGridworld(spec=make_spec(T.POGO, 45), num_envs=n, seed=4)
    t45.reset()
    with pytest.raises(MapsTooLarge, match='needs 165648 B of LDS'):
        t45.lidar_configure(num_beams=10, dtype=np.int32)
    s = t45.snapshot(n)
    s.save()
    with pytest.raises(MapsTooLarge, match='map_size 45.*needs 165648 B'):
        s.playout(np.arange(n), 3, SEED, observe='lidar')
    t45.lidar_configure(num_beams=8, dtype=np.int32)               # the world-frame form has no table: 45 x 45 is served
    assert (s.playout(np.arange(n), 3, SEED, observe='lidar').obs[0] == s.lidar_observation()).all()
    t45.close()
    # where only rewards and masks are asked for the launch has the path form's layout: an env without a lidar serves them, and says so for the rows
    ok.close()
    v2 = VecNovelGridworld(spec=T.build_spec('add32'), num_envs=n, seed=1)
    v2.reset()
    s2 = v2.snapshot(n)
    s2.save()
    r = s2.playout(np.arange(n), 3, SEED, rewards=True, masks=True)
    assert (r.rewards.sum(0) == r.ret).all() and r.obs is None
    with pytest.raises(ValueError, match='lidar_configure'):
        s2.playout(np.arange(n), 3, SEED, observe='lidar')
    v2.close()
