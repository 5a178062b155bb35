"""Trajectories that observe AgentMap views on the MI355X (observe='agent_view': csrc/ngw_traj.inc traj_view_rows in the TRAJ forms of
ngw_slot_rollout_kernel / ngw_playout_kernel, include/ngw.h ngw_snapshot_rollout_traj_views / ngw_snapshot_playout_traj_views), held to the CPU oracle
(tests/trajectory_view_oracle.py: the oracle's steps on a host copy of the parents' rows and its agent_view on the parent and on every visited row -
never the device's own step or view).  Everything is an integer and compared bit for bit.

Inputs: test_trajectories.py's recipe - 20 envs, 10 warm-up steps, autoreset with a horizon of 6 and the step counters spread over the horizon (the
plain fire10h ends pairs by deaths), the same parents, plans and weights per shape.  The oracle side of every input condition needs no GPU and was
checked on the CPU when the seeds were chosen; every test asserts them again:
  every shape with T = 5 holds a pair that ends before T and one that runs all T steps;
  each (configuration, view_size) at (65, 5) and (200, 9) holds executed steps whose agent_map differs from the block before it;
  add32 at view_size 5 holds windows fully inside the map and windows clipped by its edge.
Configurations: pogo10 (at view_size 5 every window crosses the edge of a 10 x 10 map), pogo13 (odd S: map rows are not dword-aligned), axe10 (a
pick-up changes cells next to the agent), fire10h plain (deaths give zero rows behind an end), add32 (32 x 32: windows both clipped and inside).
view_size 1 gives W * W = 9, where a 16-byte piece of the tile spans three rows; 5 is the reference's; 6 gives W * W = 169."""
import functools

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
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.playout import PlayoutTraj
from gym_novel_gridworlds_amd.snapshot import MapsTooLarge, transitions
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from gym_novel_gridworlds_amd.vec_env import RolloutTraj
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
STATE_KEYS = PO.STATE_KEYS
SEED = 0x5EED0123456789AB
N = 20
HORIZON = 6
SHAPES = ((1, 1), (65, 5), (200, 9))                            # (pairs, T): a lone lane / one past a wave / a ragged last wave, repeated parents
# configuration, autoreset with a horizon of 6, the view sizes
CONFIGS = [('pogo10', True, (1, 5, 6)), ('pogo13', True, (1, 5)), ('axe10', True, (1, 5)), ('fire10h', False, (1, 5)), ('add32', True, (1, 5, 6))]
KINDS = ('playout', 'weighted', 'rollout')


@functools.lru_cache(maxsize=None)
def twin(cfg, auto, n=N, warm=10):
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
    return spec, o, seed, kw, warmup


def make(cfg, auto, n=N, lidar=None):
    """The device twin; no lidar is configured unless `lidar` (keywords of lidar_configure) asks for one."""
    spec, o, seed, kw, warmup = twin(cfg, auto, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
    v.reset()
    for a in warmup:
        v.step(a)
    if auto:
        v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    if lidar is not None:
        v.lidar_configure(OO.lidar_config(cfg), **lidar)
    return spec, v, o


def case_inputs(spec, n, count, steps, salt=0):
    """The parents (with repeats), the plans [count, T] and the weights of one shape: a function of the shape alone."""
    rs = np.random.RandomState(1000 * salt + 7 * count + steps)
    A = len(spec.actions_id)
    return rs.randint(0, n, count), rs.randint(0, A, (count, steps)), SO.random_weights(rs, 1, A)[0]


@functools.lru_cache(maxsize=None)
def expected(cfg, auto, count, steps, salt=0):
    """The oracle's side of one shape for the three calls, computed once and shared (nobody writes to it)
    -> (parents, plans, weights, {kind: oracle_traj's dict with 'actions' [T, count]})."""
    spec, o, _, _, _ = twin(cfg, auto)
    parents, plans, x = case_inputs(spec, N, count, steps, salt)
    hz = HORIZON if auto else 0
    _, _, acts_u, _ = PO.oracle_playout(spec, o.st, parents, steps, SEED, 0, auto, hz)
    _, _, acts_w, _ = SO.oracle_weighted_playout(spec, o.st, parents, steps, SEED, x, 0, auto, hz)
    out = {}
    for kind, acts in (('playout', acts_u), ('weighted', acts_w), ('rollout', plans.T)):
        out[kind] = TO.oracle_traj(spec, o.st, parents, acts, None, auto, hz)
        out[kind]['actions'] = acts
    return parents, plans, x, out


@functools.lru_cache(maxsize=None)
def expected_views(cfg, auto, count, steps, kind, V, salt=0):
    spec, o, _, _, _ = twin(cfg, auto)
    parents, _, _, exp = expected(cfg, auto, count, steps, salt)
    return VO.expect_views(spec, o.st, parents, exp[kind], V)


def input_conditions(cfg, auto, sizes):
    """What the oracle's paths must contain for the tests to be about anything (needs no GPU)."""
    spec = twin(cfg, auto)[0]
    for count, steps in SHAPES:
        parents, _, _, exp = expected(cfg, auto, count, steps)
        if steps == 5:
            rep = exp['playout']['reports']
            assert (rep['ended'] & (rep['length'] < steps)).any() and (rep['length'] == steps).any(), (cfg, 'the T = 5 playouts need both a short and a full pair')
        if count > 1:
            for V in sizes:
                for kind in ('playout', 'rollout'):                 # (the weighted playouts of the two pogo configurations never leave their cell)
                    moved = VO.windows_move(expected_views(cfg, auto, count, steps, kind, V), exp[kind]['reports']['length'])
                    assert moved > 0, "%s V=%d %s (%d, %d): no executed step changes the window: re-emitting the parents' would pass" % (cfg, V, kind, count, steps)
            if cfg == 'add32':
                e = exp['playout']
                locs = np.concatenate([np.asarray(s['loc']).reshape(-1, 2) for s in e['states'].values()])
                inside, clipped = VO.clipped_and_inside(None, spec, 5, locs)
                assert inside > 0 and clipped > 0, "add32 (%d, %d): %d windows inside the map, %d clipped" % (count, steps, inside, clipped)


def assert_result(got, e, views, where, kids_rows=None):
    if hasattr(got.ret, 'data_ptr'):                                # a result on the device: the same bits on the host
        got = type(got)(*[None if x is None else OO.host(x) for x in got])._replace(info=OO.host(got.info).view(np.uint32))
    RO.assert_reports(got, e['reports'], where)
    if getattr(got, 'actions', None) is not None:
        assert (got.actions == e['actions']).all(), where
    TO.assert_traj(got, e, where, [k for k in ('rewards', 'masks') if getattr(got, k, None) is not None])
    if got.keys is not None:
        KO.assert_keys(got.keys, e['keys'], where)
    VO.assert_views(got.obs, views, where)
    if kids_rows is not None:
        RO.assert_rows(kids_rows[0].state(), e['ends'], where, idx=kids_rows[1])


@pytest.mark.parametrize('cfg,auto,sizes', CONFIGS)
def test_against_the_oracle(cfg, auto, sizes):
    """Playout, weighted playout and rollout at every shape and view size on an env with NO lidar configured: with and without path keys, recorded
    actions and kept children, from the same pool, from the envs and from another pool (the three hold the same rows: one oracle run serves them)."""
    input_conditions(cfg, auto, sizes)
    spec, v, o = make(cfg, auto)
    assert v.lidar is None
    n, cap = v.num_envs, 512
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    for count, steps in SHAPES:
        parents, plans, x, exp = expected(cfg, auto, count, steps)
        kids = n + np.random.RandomState(count).permutation(cap - n)[:count]
        for V in sizes:
            where = '%s auto=%d count=%d T=%d V=%d ' % (cfg, auto, count, steps, V)
            view = lambda kind: expected_views(cfg, auto, count, steps, kind, V)                      # noqa: E731
            p = pool.playout(parents, steps, SEED, kids, record=True, rewards=True, masks=True, path_keys=True, observe='agent_view', view_size=V)
            assert isinstance(p, PlayoutTraj) and p.obs['agent_map'].dtype == np.int8 and p.obs['agent_map'].shape == (steps + 1, count, 2 * V + 1, 2 * V + 1)
            assert_result(p, exp['playout'], view('playout'), where + 'playout, keys, record, children', (pool, kids))
            w = pool.playout(parents, steps, SEED, weights=x, from_envs=True, observe='agent_view', view_size=V)
            assert w.rewards is None and w.masks is None and w.keys is None and w.actions is None
            assert_result(w, exp['weighted'], view('weighted'), where + 'weighted, from the envs, views alone')
            r = pool.rollout(parents, plans, source=other, rewards=True, observe='agent_view', view_size=V)
            assert isinstance(r, RolloutTraj) and r.keys is None
            assert_result(r, exp['rollout'], view('rollout'), where + 'rollout, another pool')
            r = pool.rollout(parents, plans, kids, path_keys=True, observe='agent_view', view_size=V)
            assert r.rewards is None
            assert_result(r, exp['rollout'], view('rollout'), where + 'rollout, keys, children', (pool, kids))
    # the rows are the rows the slot observation returns: same keys, dtypes, layout
    one = pool.agent_view(np.arange(n), view_size=sizes[-1])
    p = pool.playout(np.arange(n), 1, SEED, observe='agent_view', view_size=sizes[-1])
    for k in VO.FIELDS:
        assert one[k].dtype == p.obs[k].dtype and one[k].shape == p.obs[k].shape[1:] and (one[k] == p.obs[k][0]).all(), k
    assert v.error_flags() == 0
    v.close()


def test_limits_device_results_and_unchanged_outputs():
    """Limits give the prefix; device=True gives the host's bits; adding observe='agent_view' changes no other output and no kept child."""
    import torch
    cfg, auto, V = 'axe10', True, 5
    spec, v, o = make(cfg, auto)
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n + 2 * count)
    pool.save(slots=np.arange(n))
    parents, plans, x, exp = expected(cfg, auto, count, steps)
    rs = np.random.RandomState(4)
    limits = rs.randint(0, steps + 1, count)
    limits[:4] = [0, steps, 0, 1]
    cut_rows = np.arange(steps + 1)[:, None] > limits[None, :]
    kids_a, kids_b = n + np.arange(count), n + count + np.arange(count)
    calls = (('playout', lambda **k: pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, path_keys=True, **k)),
             ('weighted', lambda **k: pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, weights=x, **k)),
             ('rollout', lambda **k: pool.rollout(parents, plans, rewards=True, path_keys=True, **k)))
    for kind, call in calls:
        views = expected_views(cfg, auto, count, steps, kind, V)
        whole = call(observe='agent_view', view_size=V, children=kids_a)
        assert_result(whole, exp[kind], views, kind)
        # the same call without the keyword: every other field and every kept child is identical
        bare = call(children=kids_b)
        assert bare.obs is None
        for name in whole._fields:
            if name != 'obs' and whole[name] is not None:
                assert (whole[name] == bare[name]).all(), (kind, name)
        st = pool.state()
        assert all((np.asarray(st[k])[kids_a] == np.asarray(st[k])[kids_b]).all() for k in STATE_KEYS), kind
        # limits: the prefix, zeros behind it, block 0 even at a limit of 0
        part = call(observe='agent_view', view_size=V, limits=limits)
        e = TO.oracle_traj(spec, o.st, parents, exp[kind]['actions'], limits, auto, HORIZON)
        assert e['events']['limited'] > 0
        e['actions'] = np.where(cut_rows[1:], -1, exp[kind]['actions'])
        assert_result(part, e, VO.expect_views(spec, o.st, parents, e, V), 'limited ' + kind)
        for k in VO.FIELDS:
            shape = cut_rows.shape + (1,) * (whole.obs[k].ndim - 2)
            assert (part.obs[k] == np.where(cut_rows.reshape(shape), 0, whole.obs[k])).all(), (kind, k)
        assert part.obs['agent_map'][0, limits == 0].any()
    # on the device: the fields stay there, in torch's types, ordered behind the launch
    d = pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, observe='agent_view', view_size=V, device=True)
    assert d.obs['agent_map'].dtype == torch.int8 and d.obs['agent_facing_id'].dtype == torch.int32 and d.obs['inventory_items_quantity'].dtype == torch.int32
    assert all(x.is_cuda and tuple(x.shape[:2]) == (steps + 1, count) for x in d.obs.values())
    t, j = transitions(d)
    assert int(t.numel()) == int(exp['playout']['reports']['length'].sum())
    views = expected_views(cfg, auto, count, steps, 'playout', V)
    assert (d.obs['agent_map'][t + 1, j].cpu().numpy() == views['agent_map'][t.cpu().numpy() + 1, j.cpu().numpy()]).all()
    assert_result(d, exp['playout'], views, 'device')
    dr = pool.rollout(parents, plans, observe='agent_view', view_size=V, device=True)
    assert_result(dr, exp['rollout'], expected_views(cfg, auto, count, steps, 'rollout', V), 'device rollout')
    assert v.error_flags() == 0
    v.close()


def test_a_bad_parent_gives_zero_rows_in_every_block_and_its_neighbours_are_unaffected():
    import torch
    cfg, auto, V = 'axe10', True, 5
    spec, v, o = make(cfg, auto)
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
    p = pool.playout(dev, steps, SEED, record=True, rewards=True, masks=True, observe='agent_view', view_size=V)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    r = pool.rollout(dev, acts, rewards=True, observe='agent_view', view_size=V)
    assert v.error_flags() == F_BAD_INDEX
    _, _, au, _ = PO.oracle_playout(spec, o.st, parents, steps, SEED, 0, True, HORIZON)
    eu = TO.oracle_traj(spec, o.st, parents, au, None, True, HORIZON)
    er = TO.oracle_traj(spec, o.st, parents, plans.T, None, True, HORIZON)
    for res, e in ((p, eu), (r, er)):
        views = VO.expect_views(spec, o.st, parents, e, V)
        assert views['agent_map'][0, ~good].any()                     # (the oracle's rows for the replaced parents are not zero: the zeros below are the kernel's)
        for k in VO.FIELDS:
            assert (res.obs[k][:, good] == views[k][:, good]).all(), k
            assert not res.obs[k][:, ~good].any(), k                  # block 0 included
        assert (res.rewards[:, good] == e['rewards'][:, good]).all() and not res.rewards[:, ~good].any()
        for k in ('ret', 'length', 'ended', 'info'):
            assert (res[k][good] == e['reports'][k][good]).all() and (res[k][~good] == 0).all(), k
    v.close()


def test_with_a_lidar_configured_both_observations_agree_and_nothing_is_committed():
    cfg, auto, V = 'pogo13', True, 5
    spec, v, o = make(cfg, auto, lidar=dict(fused=True, dtype=np.int32))
    n, count, steps = v.num_envs, 200, 9
    pool = v.snapshot(n)
    pool.save()
    parents, plans, x, exp = expected(cfg, auto, count, steps)
    lc = v.lidar
    cols = [spec.items_id[item] for item in lc.inventory_order(spec)]
    tail = lc.num_beams * len(lc.lidar_items_id)
    env_obs = v.lidar_observation(copy=True)
    before = [np.asarray(x).copy() for x in (pool.state()[k] for k in STATE_KEYS)] + [np.asarray(x).copy() for x in (v.get_state()[k] for k in sorted(v.get_state()))]
    for kind, call in (('playout', lambda **k: pool.playout(parents, steps, SEED, record=True, rewards=True, masks=True, path_keys=True, **k)),
                       ('rollout', lambda **k: pool.rollout(parents, plans, rewards=True, path_keys=True, from_envs=True, **k))):
        a, b = call(observe='agent_view', view_size=V), call(observe='lidar')
        assert_result(a, exp[kind], expected_views(cfg, auto, count, steps, kind, V), kind + ' with a fused lidar')
        for name in a._fields:
            if name != 'obs' and a[name] is not None:
                assert (a[name] == b[name]).all(), (kind, name)
        # the inventory is in both observations: the lidar row's tail is the view's inventory in the wrapper's item order; zero rows in the same places
        assert (b.obs[..., tail:] == a.obs['inventory_items_quantity'][..., cols]).all(), kind
        ran = np.arange(steps + 1)[:, None] <= a.length[None, :]
        assert not a.obs['agent_map'][~ran].any() and not b.obs[~ran].any() and a.obs['agent_map'][ran].any()
    after = [np.asarray(x) for x in (pool.state()[k] for k in STATE_KEYS)] + [np.asarray(x) for x in (v.get_state()[k] for k in sorted(v.get_state()))]
    assert all((p == q).all() for p, q in zip(before, after)) and (v.lidar_observation() == env_obs).all()
    assert v.error_flags() == 0
    v.close()


def test_other_surfaces():
    """venv.playouts [T + 1, N, P, ...] and the single-env adapter [T + 1, P, ...]."""
    spec, v, o = make('pogo10', True, n=3)
    P, steps, V = 2, 3, 2
    par = np.repeat(np.arange(3), P)
    _, rep, acts, _ = PO.oracle_playout(spec, o.st, par, steps, SEED, 0, True, HORIZON)
    e = TO.oracle_traj(spec, o.st, par, acts, None, True, HORIZON)
    views = VO.expect_views(spec, o.st, par, e, V)
    got = v.playouts(P, steps, SEED, rewards=True, masks=True, observe='agent_view', view_size=V)
    K = len(spec.items_id)
    assert isinstance(got, PlayoutTraj) and got.rewards.shape == (steps, 3, P) and got.obs['agent_map'].shape == (steps + 1, 3, P, 2 * V + 1, 2 * V + 1)
    assert got.obs['agent_facing_id'].shape == (steps + 1, 3, P) and got.obs['inventory_items_quantity'].shape == (steps + 1, 3, P, K)
    VO.assert_views({k: x.reshape((steps + 1, 3 * P) + x.shape[3:]) for k, x in got.obs.items()}, views, 'venv.playouts')
    assert (got.length.reshape(-1) == rep['length']).all() and (got.rewards.reshape(steps, -1) == e['rewards']).all()
    v.close()
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    vec = env.unwrapped._backend()
    rows = vec.get_state()
    P, steps = 5, 3
    play = env.playouts(P, steps, SEED, rewards=True, observe='agent_view')
    _, _, acts, _ = PO.oracle_playout(vec.spec, rows, np.zeros(P, np.int64), steps, SEED)
    e = TO.oracle_traj(vec.spec, rows, np.zeros(P, np.int64), acts)
    assert play.obs['agent_map'].shape == (steps + 1, P, 11, 11)
    VO.assert_views(play.obs, VO.expect_views(vec.spec, rows, np.zeros(P, np.int64), e, 5), 'adapter')
    assert (play.rewards == e['rewards']).all()
    env.close()


def test_map_limits():
    """The views run under the handle's rollout layout, with the inventory shadows only where keys are asked for, so they keep the path form's map
    limit and - without keys - even the plain calls'.  Pogostick 47 x 47 (the largest the plain calls serve) serves views with keys; 48 x 48 is refused,
    the text starting with "map_size" and naming the bytes of the maps and inventories (64 * 2308 + 64 * 4 * 9; the handle keeps no rollout layout
    there, and rewards alone are refused too: no handle serves rewards alone and not the views).
    With a fused int32 lidar of 8 beams the handle's own layout grows: at 45 x 45 it takes 162 128 B, the shadows 2 304 B more - the views run, the
    views with keys answer MapsTooLarge naming 164 432 B."""
    n = 4
    big = VecNovelGridworld(spec=make_spec(T.POGO, 47), num_envs=n, seed=4)
    big.reset()
    s = big.snapshot(2 * n)
    s.save(slots=np.arange(n))
    kids = n + np.arange(n)
    r = s.rollout(np.arange(n), np.zeros((n, 1), np.int64), kids, observe='agent_view', path_keys=True, rewards=True)
    p = s.playout(np.arange(n), 3, SEED, observe='agent_view', view_size=8, masks=True)
    for k in VO.FIELDS:
        assert (r.obs[k][0] == s.agent_view(np.arange(n))[k]).all() and (r.obs[k][1] == s.agent_view(kids)[k]).all(), k
        assert (p.obs[k][0] == s.agent_view(np.arange(n), view_size=8)[k]).all(), k
    assert r.obs['agent_map'].any() and big.error_flags() == 0
    big.close()
    huge = VecNovelGridworld(spec=make_spec(T.POGO, 48), num_envs=n, seed=4)
    huge.reset()
    for call in (lambda: huge.playouts(2, 3, SEED, observe='agent_view'),
                 lambda: huge.playouts(2, 3, SEED, observe='agent_view', path_keys=True, rewards=True),
                 lambda: huge.playouts(2, 3, SEED, observe='agent_view', view_size=1)):
        with pytest.raises(MapsTooLarge, match=r'^map_size 48.* take 150016 B'):
            call()
    with pytest.raises(MapsTooLarge, match='^map_size 48'):
        huge.playouts(2, 3, SEED, rewards=True)
    huge.close()
    f45 = VecNovelGridworld(spec=make_spec(T.POGO, 45), num_envs=n, seed=4)
    f45.reset()
    f45.lidar_configure(num_beams=8, fused=True, dtype=np.int32)
    fs = f45.snapshot(2 * n)
    fs.save(slots=np.arange(n))
    r = fs.rollout(np.arange(n), np.zeros((n, 1), np.int64), kids, observe='agent_view', rewards=True)
    for k in VO.FIELDS:
        assert (r.obs[k][0] == fs.agent_view(np.arange(n))[k]).all() and (r.obs[k][1] == fs.agent_view(kids)[k]).all(), k
    for call in (lambda: fs.playout(np.arange(n), 3, SEED, observe='agent_view', path_keys=True),
                 lambda: fs.rollout(np.arange(n), np.zeros((n, 3), np.int64), observe='agent_view', path_keys=True)):
        with pytest.raises(MapsTooLarge, match=r'^map_size 45.* need 164432 B'):
            call()
    assert f45.error_flags() == 0
    f45.close()
