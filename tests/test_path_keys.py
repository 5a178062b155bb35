"""Path keys and per-pair step limits on the MI355X (csrc/ngw_path.inc, the PATH forms of ngw_slot_rollout_kernel / ngw_playout_kernel,
include/ngw.h ngw_snapshot_rollout_path / ngw_snapshot_playout_path), held to the CPU oracle (tests/path_key_oracle.py: the oracle's steps
on a host copy of the parents' rows, state_keys.keys_of_rows of the row after every executed step - never the device's own step, mask or key).
Everything is an integer and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import expand_oracle as XO
import ngw_testlib as T
import path_key_oracle as KO
import playout_oracle as PO
import sample_oracle as SO
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd import LimitActions, VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.playout import Playout, PlayoutPath
from gym_novel_gridworlds_amd.snapshot import fresh_steps
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX
from gym_novel_gridworlds_amd.state_keys import KEY_ALL, KEY_INV, KEY_MAP, KEY_POSE, KEY_STATE
from gym_novel_gridworlds_amd.vec_env import PlanEval, RolloutPath
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
STATE_KEYS = PO.STATE_KEYS
SEED = 0x5EED0123456789AB
SHAPES = ((1, 1), (65, 5), (200, 9))                            # (pairs, T): a lone lane / one past a wave / a ragged last wave
# configuration, autoreset with a horizon of 6, warm-up steps, fields, the event the oracle must see inside the paths
CONFIGS = [('pogo10', False, 10, KEY_STATE, 'map_writes'), ('pogo13', False, 10, KEY_STATE, 'map_writes'), ('axe10', False, 10, KEY_STATE, 'pickups'),
           ('crate11e', False, 10, KEY_STATE, 'inv_jumps'), ('fencer10m', False, 10, KEY_ALL, 'double_counts'), ('fire10h', False, 10, KEY_STATE, 'deaths'),
           ('fire10h', True, 10, KEY_ALL, 'cuts'), ('add32', False, 10, KEY_STATE, 'map_writes')]


def twin(cfg, n=20, auto=False, warm=10):
    """The oracle after `warm` random steps (autoreset with a horizon of 6 where `auto`), and what a device env needs to be its twin."""
    spec = T.build_spec(cfg)
    seed = XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=6) if auto else {}
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    o.reset()
    rs = np.random.RandomState(n + warm)
    warmup = [rs.randint(0, len(spec.actions_id), n).astype(np.int32) for _ in range(warm)]
    for a in warmup:
        o.step(a)
    return spec, o, seed, kw, warmup


def make(cfg, n=20, auto=False, warm=10):
    spec, o, seed, kw, warmup = twin(cfg, n, auto, warm)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    v.reset()
    for a in warmup:
        v.step(a)
    return spec, v, o


def case_inputs(spec, n, count, steps, salt=0):
    """The parents (with repeats), the plans [count, T] and the weights of one shape: a function of the shape alone."""
    rs = np.random.RandomState(1000 * salt + 7 * count + steps)
    A = len(spec.actions_id)
    return rs.randint(0, n, count), rs.randint(0, A, (count, steps)), SO.random_weights(rs, 1, A)[0]


def expected(spec, o, count, steps, fields, salt=0):
    """The oracle's side of one shape for the three calls -> {kind: (actions [T, count], keys, reports, ends, events)}."""
    parents, plans, x = case_inputs(spec, len(o.st.facing), count, steps, salt)
    auto, hz = bool(o.autoreset), int(o.horizon)
    _, _, acts_u, _ = PO.oracle_playout(spec, o.st, parents, steps, SEED, 0, auto, hz)
    _, _, acts_w, _ = SO.oracle_weighted_playout(spec, o.st, parents, steps, SEED, x, 0, auto, hz)
    out = {}
    for kind, acts in (('playout', acts_u), ('weighted', acts_w), ('rollout', plans.T)):
        out[kind] = (acts,) + KO.oracle_path(spec, o.st, parents, acts, None, auto, hz, fields)
    return parents, plans, x, out


def host_keys(k):
    return k.cpu().numpy().view(np.uint64) if hasattr(k, 'data_ptr') else k


@pytest.mark.parametrize('cfg,auto,warm,fields,event', CONFIGS)
def test_keys_against_the_oracle(cfg, auto, warm, fields, event):
    """Rollout, playout and weighted playout at every shape, from the same pool with repeated parents, from the envs and from another pool
    (the three hold the same rows, so one oracle run serves them).  The oracle must have met the configuration's event inside the paths."""
    spec, v, o = make(cfg, auto=auto, warm=warm)
    n, cap = v.num_envs, 512
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    seen = 0
    for count, steps in SHAPES:
        parents, plans, x, exp = expected(spec, o, count, steps, fields)
        kids = n + np.random.RandomState(count).permutation(cap - n)[:count] if steps == 5 else None
        for src, kw in (('same pool', {}), ('from the envs', dict(from_envs=True)), ('another pool', dict(source=other))):
            where = '%s auto=%d count=%d T=%d %s' % (cfg, auto, count, steps, src)
            for kind in ('playout', 'weighted'):
                acts, keys, rep, ends, _, ev = exp[kind]
                p = pool.playout(parents, steps, SEED, kids, record=True, path_keys=True, fields=fields, weights=x if kind == 'weighted' else None, **kw)
                assert isinstance(p, PlayoutPath)
                RO.assert_reports(p, rep, where + ' ' + kind)
                assert (p.actions == acts).all(), where
                KO.assert_keys(p.keys, keys, where + ' ' + kind)
                if kids is not None:
                    RO.assert_rows(pool.state(), ends, where, idx=kids)
            acts, keys, rep, ends, _, ev = exp['rollout']
            r = pool.rollout(parents, plans, kids, path_keys=True, fields=fields, **kw)
            assert isinstance(r, RolloutPath)
            RO.assert_reports(r, rep, where + ' rollout')
            KO.assert_keys(r.keys, keys, where + ' rollout')
            if kids is not None:
                RO.assert_rows(pool.state(), ends, where, idx=kids)
        seen += sum(exp[kind][5][event] for kind in exp)
        assert all(((exp[kind][1] != 0).sum(0) == exp[kind][2]['length']).all() for kind in exp)
    assert seen > 0, "%s: the oracle met no '%s' inside the paths: the inputs are wrong" % (cfg, event)
    assert v.error_flags() == 0
    v.close()


def test_fields_selections_and_refusals():
    import torch
    spec, v, o = make('pogo13')
    pool = v.snapshot(v.num_envs)
    pool.save()
    count, steps = 65, 5
    for fields in (KEY_POSE | KEY_INV, KEY_ALL, KEY_MAP):
        parents, plans, x, exp = expected(spec, o, count, steps, fields)
        KO.assert_keys(pool.playout(parents, steps, SEED, path_keys=True, fields=fields).keys, exp['playout'][1], 'fields=%d playout' % fields)
        KO.assert_keys(pool.rollout(parents, plans, path_keys=True, fields=fields).keys, exp['rollout'][1], 'fields=%d rollout' % fields)
    for bad in (0, 64):
        with pytest.raises(ValueError):
            pool.playout(parents, steps, SEED, path_keys=True, fields=bad)
        with pytest.raises(ValueError):
            pool.rollout(parents, plans, path_keys=True, fields=bad)
    # ... and by the library itself
    L, N = _cabi.lib(), None
    buf = torch.zeros(steps * 8, dtype=torch.int64, device='cuda')
    acts = torch.zeros(steps * 8, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    k, a = C.c_void_p(buf.data_ptr()), C.c_void_p(acts.data_ptr())
    for bad in (0, 64):
        assert L.ngw_snapshot_playout_path(v._h, pool._s, N, 8, steps, 1, 0, N, N, N, N, N, N, N, N, N, N, 0, bad, k, 8) == _cabi.E_INVALID_ARG
        assert 'key fields' in _cabi.last_error()
        assert L.ngw_snapshot_rollout_path(v._h, pool._s, N, a, 8, steps, N, N, N, 8, N, N, N, N, bad, k, 8) == _cabi.E_INVALID_ARG
    assert L.ngw_snapshot_playout_path(v._h, pool._s, N, 8, steps, 1, 0, N, N, N, N, N, N, N, N, N, N, 0, 15, k, 7) == _cabi.E_INVALID_ARG
    assert 'key stride of 7' in _cabi.last_error()
    assert L.ngw_snapshot_rollout_path(v._h, pool._s, N, a, 8, steps, N, N, N, 8, N, N, N, N, 15, k, 8) == 0      # keys alone are a result
    v.sync()
    assert (buf.cpu().numpy() != 0).all() and v.error_flags() == 0
    v.close()


def test_device_cross_check_a_limited_replay_lands_on_the_keyed_state():
    """keys[t, j] equals snap.keys() of the child a rollout of pair j's recorded actions leaves with limits = t + 1."""
    import torch
    spec, v, o = make('axe10', auto=True)
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n + 64)
    pool.save(slots=np.arange(n))
    parents = torch.from_numpy(np.random.RandomState(1).randint(0, n, count).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    play = pool.playout(parents, steps, SEED, record=True, path_keys=True, device=True)
    assert play.keys.dtype == torch.int64 and tuple(play.keys.shape) == (steps, count)
    keys = host_keys(play.keys)
    ts, js = np.nonzero(keys)
    pick = np.random.RandomState(2).permutation(len(ts))[:40]
    pick = np.concatenate([pick, [np.argmax(ts)]])                   # (a last step among them)
    ts, js = ts[pick], js[pick]
    kids = n + np.arange(len(pick))
    r = pool.rollout(parents[torch.from_numpy(js).cuda()].contiguous(), play.actions[:, torch.from_numpy(js).cuda()].contiguous(),
                     torch.from_numpy(kids.astype(np.int32)).cuda(), limits=ts + 1)
    assert isinstance(r, PlanEval) and not isinstance(r, RolloutPath) and (r.length == ts + 1).all()
    assert (pool.keys(kids) == keys[ts, js]).all()
    assert v.error_flags() == 0
    v.close()


def test_limits():
    """A limited playout is the prefix of the unlimited one - reports, actions, keys, children against oracle rows; limit 0 leaves a copy of the
    parent; a pair cut by its limit is not ended; a device tensor with -3 and T + 5 behaves as 0 and T."""
    import torch
    spec, v, o = make('fire10h', auto=True)
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n + count)
    pool.save(slots=np.arange(n))
    rows = pool.state()
    rs = np.random.RandomState(4)
    parents = rs.randint(0, n, count)
    kids = n + np.arange(count)
    limits = rs.randint(0, steps + 1, count)
    limits[:4] = [0, steps, 0, 1]
    whole = pool.playout(parents, steps, SEED, record=True, path_keys=True)
    keys, rep, ends, _, ev = KO.oracle_path(spec, rows, parents, whole.actions, limits, True, 6)
    assert ev['limited'] > 0 and ev['deaths'] + ev['cuts'] > 0
    cut = np.arange(steps)[:, None] >= limits[None, :]
    for x in (None, SO.random_weights(rs, 1, len(spec.actions_id))[0]):
        if x is not None:
            whole = pool.playout(parents, steps, SEED, record=True, path_keys=True, weights=x)
            keys, rep, ends, _, ev = KO.oracle_path(spec, rows, parents, whole.actions, limits, True, 6)
        part = pool.playout(parents, steps, SEED, kids, record=True, path_keys=True, limits=limits, weights=x)
        RO.assert_reports(part, rep, 'limited playout')
        assert (part.actions == np.where(cut, -1, whole.actions)).all() and (part.first_action == part.actions[0]).all()
        KO.assert_keys(part.keys, keys, 'limited playout')
        assert (part.keys == np.where(cut, np.uint64(0), whole.keys)).all()
        RO.assert_rows(pool.state(), ends, 'limited playout', idx=kids)
        shorter = limits < whole.length
        assert shorter.any() and not part.ended[shorter].any() and (part.length[shorter] == limits[shorter]).all()
        zero = limits == 0
        assert (part.ret[zero] == 0).all() and (part.info[zero] == 0).all() and (part.length[zero] == 0).all()
        st = pool.state()
        for k in STATE_KEYS:
            assert (st[k][kids[zero]] == rows[k][parents[zero]]).all(), k
        # limits alone: the old result type
        only = pool.playout(parents, steps, SEED, limits=limits, weights=x)
        assert isinstance(only, Playout) and not isinstance(only, PlayoutPath) and (only.length == part.length).all()
    # the rollout of the recorded actions under the same limits, the limits as a device tensor with values outside [0, T]
    wild = limits.copy()
    wild[limits == 0], wild[limits == steps] = -3, steps + 5
    acts = torch.from_numpy(np.ascontiguousarray(whole.actions)).cuda()
    dev = torch.from_numpy(wild.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    r = pool.rollout(parents, acts, kids, limits=dev, path_keys=True)
    RO.assert_reports(r, rep, 'limited rollout')
    KO.assert_keys(r.keys, keys, 'limited rollout')
    RO.assert_rows(pool.state(), ends, 'limited rollout', idx=kids)
    with pytest.raises(ValueError, match='outside'):
        pool.rollout(parents, acts, kids, limits=wild)
    assert v.error_flags() == 0
    v.close()


def test_a_bad_index_gives_a_column_of_zero_keys():
    import torch
    spec, v, o = make('axe10')
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
    where = np.nonzero(good)[0]
    p = pool.playout(dev, steps, SEED, record=True, path_keys=True)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    r = pool.rollout(dev, acts, path_keys=True)
    assert v.error_flags() == F_BAD_INDEX
    for j in where[[0, 3, 4, 5, 20, -2, -1]]:                            # (the neighbours of the bad lanes among them; pair numbers are positions)
        _, _, au, _ = PO.oracle_playout(spec, pool.state(), parents[j:j + 1], steps, SEED, int(j))
        ku, repu, _, _, _ = KO.oracle_path(spec, pool.state(), parents[j:j + 1], au)
        KO.assert_keys(p.keys[:, j:j + 1], ku, 'playout pair %d' % j)
        assert p.ret[j] == repu['ret'][0] and p.length[j] == repu['length'][0]
    kr, repr_, _, _, _ = KO.oracle_path(spec, pool.state(), parents[good], plans[good].T)
    KO.assert_keys(r.keys[:, good], kr, 'rollout, the other pairs')
    RO.assert_reports(PlanEval(*[x[good] for x in r[:4]]), repr_, 'rollout, the other pairs')
    for res in (p, r):
        assert (res.keys[:, ~good] == 0).all()
        for k in ('ret', 'length', 'ended', 'info'):
            assert (res[k][~good] == 0).all(), k
    v.close()


def test_the_closed_loop_archives_every_new_state_of_the_paths():
    """playout -> table.insert -> fresh_steps -> limited rollout into archive slots, all on the device: every archived row is the oracle's state at
    that (t, j), the archived keys are pairwise distinct and in the table; the oracle shows revisits, so `fresh` is not all True."""
    import torch
    spec, v, o = make('pogo10')
    n, count, steps = v.num_envs, 64, 9
    pool = v.snapshot(n)
    pool.save()
    rows = pool.state()
    parents = torch.full((count,), 3, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    play = pool.playout(parents, steps, SEED, record=True, path_keys=True, device=True)
    table = v.key_table(2 * steps * count)
    found = table.insert(play.keys.reshape(-1), device=True)
    fresh = found.fresh.reshape(steps, count)
    t, j = fresh_steps(fresh)
    m = int(t.numel())
    archive = v.snapshot(m)
    slots = torch.arange(m, dtype=torch.int32, device='cuda')
    r = archive.rollout(parents[j].contiguous(), play.actions[:, j].contiguous(), slots, source=pool, limits=(t + 1).to(torch.int32).contiguous(), device=True)
    th, jh = t.cpu().numpy(), j.cpu().numpy()
    assert (r.length.cpu().numpy() == th + 1).all()
    keys, _, _, states, _ = KO.oracle_path(spec, rows, np.full(count, 3), play.actions.cpu().numpy())
    KO.assert_keys(host_keys(play.keys), keys, 'closed loop')
    nz = keys[keys != 0]
    assert 0 < m == len(np.unique(nz)) < nz.size, "the oracle shows no revisited state: pick another shape"
    got = archive.state()
    for i in range(m):
        for k in STATE_KEYS:
            assert (np.asarray(got[k][i]).reshape(-1) == np.asarray(states[(int(th[i]), int(jh[i]))][k]).reshape(-1)).all(), (i, k)
    akeys = archive.keys()
    assert len(np.unique(akeys)) == m and (akeys == keys[th, jh]).all()
    assert (table.lookup(akeys) >= 0).all() and len(table) == m
    # the earliest step that reached a state is the fresh one
    first = {}
    for tt in range(steps):
        for jj in range(count):
            if keys[tt, jj]:
                first.setdefault(int(keys[tt, jj]), (tt, jj))
    assert sorted(first.values()) == sorted(zip(th.tolist(), jh.tolist()))
    assert v.error_flags() == 0
    v.close()


def test_plain_calls_are_unchanged():
    spec, v, o = make('axe10', auto=True)
    n = v.num_envs
    pool = v.snapshot(n)
    pool.save()
    parents, plans, x = case_inputs(spec, n, 200, 9)
    a, b = pool.rollout(parents, plans), pool.rollout(parents, plans, limits=None, path_keys=False)
    assert type(a) is type(b) is PlanEval and all((p == q).all() for p, q in zip(a, b))
    a, b = pool.playout(parents, 9, SEED, record=True), pool.playout(parents, 9, SEED, record=True, limits=None, path_keys=False)
    assert type(a) is type(b) is Playout and all((p == q).all() for p, q in zip(a, b))
    c = pool.playout(parents, 9, SEED, record=True, path_keys=True)
    assert all((p == q).all() for p, q in zip(a, c[:6]))            # the keys change nothing else
    v.close()


def test_other_surfaces():
    """venv.playouts(path_keys=True) [T, N, P], the single-env adapter [T, P] and LimitActions, each against the oracle."""
    spec, v, o = make('pogo10', n=3, warm=4)
    P, steps = 2, 3
    par = np.repeat(np.arange(3), P)
    _, _, acts, _ = PO.oracle_playout(spec, o.st, par, steps, SEED)
    keys, rep, _, _, _ = KO.oracle_path(spec, o.st, par, acts)
    got = v.playouts(P, steps, SEED, path_keys=True)
    assert isinstance(got, PlayoutPath) and got.keys.shape == (steps, 3, P) and got.actions is None
    KO.assert_keys(got.keys.reshape(steps, -1), keys, 'venv.playouts')
    assert (got.length.reshape(-1) == rep['length']).all()
    import torch
    dev = v.playouts(P, steps, SEED, path_keys=True, fields=KEY_ALL, device=True)
    kall, _, _, _, _ = KO.oracle_path(spec, o.st, par, acts, fields=KEY_ALL)
    assert dev.keys.dtype == torch.int64
    KO.assert_keys(host_keys(dev.keys).reshape(steps, -1), kall, 'venv.playouts, device')
    v.close()
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    vec = env.unwrapped._backend()
    rows = vec.get_state()
    P, steps = 1, 1
    for who, sp in ((env, vec.spec), (LimitActions(env, {'Break', 'Forward'}), None)):
        play = who.playouts(P, steps, SEED, path_keys=True)
        sp = sp or who.__dict__['_playout_env'][2].spec
        _, _, acts, _ = PO.oracle_playout(sp, rows, np.zeros(P, np.int64), steps, SEED)
        keys, _, _, _, _ = KO.oracle_path(sp, rows, np.zeros(P, np.int64), acts)
        assert isinstance(play, PlayoutPath) and play.keys.shape == (steps, P)
        KO.assert_keys(play.keys, keys, type(who).__name__)
    who.close()
