"""The contracts on which the two kernels behind snapshot rollouts and playouts differ or must agree (csrc/ngw_slot_rollout.inc, csrc/ngw_playout.inc) -
what a merge of the two could blur -, through the C ABI with ctypes.  Every output tensor is pre-filled with a sentinel, so "stored 0" and "left alone" are
told apart; the expected values are the CPU oracles' of tests/ (never the device's own).

Shape - the smallest at which the shared parts can go wrong: the default Pogostick spec under autoreset with a horizon of 5 and the parents' step
counters spread over it, so every pair ends within 5 steps; count = 70 (a full wave and a wave with 58 lanes past `count`); T = 6 (a second Philox block
at step 4, and step 5 behind the wave-uniform exit of every wave: every tail fill runs); the pairs of the second wave limited to <= 2 steps; pair BAD
with a parent index out of range; a plan id outside the action list in a live pair and one in an ended pair; first_pair just below 2^32, so hi32(p)
changes inside the call.

test_slot_rollout.py (test_bad_indices_from_the_device_skip_their_pairs pre-fills the four reports of a rollout; test_invalid_action_ids_from_the_device
holds the no-op step) and test_playout.py (its bad-index case) already pin the two report rules one at a time; here they are asserted side by side on
the same pairs, beside the per-step outputs those tests do not pre-fill."""
import ctypes as C
import functools

import numpy as np
import pytest

import expand_oracle as XO
import guided_playout_oracle as GO
import path_key_oracle as KO
import playout_oracle as PO
import sample_oracle as SO
import slot_rollout_oracle as RO
import trajectory_oracle as TO
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd import _cabi, make_spec
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_BAD_WEIGHT, F_INVALID_ACTION
from gym_novel_gridworlds_amd.state_keys import KEY_STATE, keys_of_rows
from oracle.ngw_oracle import Oracle

N, COUNT, T, HORIZON, VIEW = 20, 70, 6, 5, 2
PAD = 128                                               # COUNT rounded up to whole waves: the stride of the view tiles
BAD = 5                                                 # the pair whose parent index is out of range
SEED, FILL_SEED, FIRST_PAIR = 0x5EEDFACE12345678, 0x7AB1E5EED0000002, (1 << 32) - 30
S32, S8, S64 = -77, 0xAB, 0x5A5A5A5A5A5A5A5A            # the sentinels


@functools.lru_cache(maxsize=None)
def twin():
    """The oracle after 10 random steps with the step counters spread over the horizon, and what a device env needs to be its twin."""
    spec = make_spec('NovelGridworld-Pogostick-v1', 10)
    seed = XO.good_seed(spec, N)
    o = Oracle(spec.compile(), N, seed=seed, autoreset=True, horizon=HORIZON)
    o.reset()
    rs = np.random.RandomState(N + 10)
    warmup = [rs.randint(0, len(spec.actions_id), N).astype(np.int32) for _ in range(10)]
    for a in warmup:
        o.step(a)
    o.st.step_count[...] = np.arange(N) % HORIZON
    return spec, o, seed, warmup


@functools.lru_cache(maxsize=None)
def inputs():
    """-> (parents for the oracle (BAD's replaced by row 0), plans [T, COUNT] with the two ids outside the list, limits, (live pair, its step), (ended
    pair, its step), default weights)."""
    spec, o, _, _ = twin()
    A = len(spec.actions_id)
    rs = np.random.RandomState(COUNT)
    parents = rs.randint(0, N, COUNT).astype(np.int32)
    parents[BAD] = 0
    plans = rs.randint(0, A, (T, COUNT)).astype(np.int32)
    limits = np.full(COUNT, T, np.int32)
    limits[[7, 20, 33]] = [1, 0, 3]
    limits[64:] = [0, 1, 2, 2, 1, 0]                    # the second wave: the early exit at step 2 at the latest
    length = RO.oracle_slot_rollout(spec, o.st, parents, plans.T, True, HORIZON)[1]['length']
    free = np.array([j for j in range(64) if j != BAD and limits[j] == T])
    live, over = free[(length[free] >= 3) & (length[free] <= 4)][0], free[length[free] == 1][0]   # (the no-op step adds one to `live`'s length: still < T)
    plans[1, live], plans[3, over] = A + 5, -7          # (step 1 of a pair that runs 3 or 4 steps; step 3 of a pair that ended at step 0)
    weights = (rs.randint(0, 4, A) * rs.randint(0, 2, A)).astype(np.float32)
    weights[rs.randint(A)] = 1.0
    return parents, plans, limits, (int(live), 1), (int(over), 3), weights


@pytest.fixture(scope='module')
def dev():
    """The device twin, a pool whose slots 0 .. N-1 hold the envs' states, and the helpers of one call."""
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld
    spec, o, seed, warmup = twin()
    v = VecNovelGridworld(spec=spec, num_envs=N, seed=seed, autoreset=True, horizon=HORIZON)
    v.reset()
    for a in warmup:
        v.step(a)
    v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    st = v.get_state()
    assert (st['map'].reshape(N, -1) == np.asarray(o.st.map).reshape(N, -1)).all() and (st['inv'] == o.st.inv).all() and (st['loc'] == o.st.loc).all()
    pool = v.snapshot(N + COUNT)
    pool.save()
    assert v.error_flags() == 0
    d = torch.device('cuda:%d' % v.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)                                     # noqa: E731
    parents = inputs()[0].copy()
    parents[BAD] = N + COUNT + 3                        # outside the pool
    box = dict(v=v, pool=pool, L=_cabi.lib(), torch=torch, d=d, up=up, parents=up(parents), kids=up(np.arange(N, N + COUNT, dtype=np.int32)))
    yield box
    v.close()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def filled(dev, shape, dtype, value):
    return dev['torch'].full(shape, value, dtype=dtype, device=dev['d'])


def reports(dev):
    t = dev['torch']
    return [filled(dev, (COUNT,), t.int32, S32), filled(dev, (COUNT,), t.int32, S32), filled(dev, (COUNT,), t.uint8, S8), filled(dev, (COUNT,), t.int32, S32)]


def flags_after(dev):
    dev['v'].sync()
    return dev['v'].error_flags()                       # (reads and clears)


def assert_reports(got, exp, rule, where):
    """ret / length / ended / info against the oracle's for every pair but BAD, and BAD by `rule`: 'untouched' (a rollout) or 'zeros' (a playout)."""
    good = np.arange(COUNT) != BAD
    g = dict(zip(('ret', 'length', 'ended', 'info'), [x.cpu().numpy() for x in got]))
    RO.assert_reports({k: x[good] for k, x in g.items()}, {k: x[good] for k, x in exp.items()}, where)
    want = (S32, S32, S8, S32) if rule == 'untouched' else (0, 0, 0, 0)
    assert tuple(int(g[k][BAD]) for k in ('ret', 'length', 'ended', 'info')) == want, "%s: the reports of the skipped pair are not %s" % (where, rule)


def per_step(got, exp, where, name, skipped):
    """A [T, COUNT] output against the oracle's, column BAD against `skipped`; nothing holds the sentinel any more."""
    g = got.cpu().numpy()
    if exp.dtype == np.uint64:
        g = g.view(np.uint64)
    e = exp.copy()
    e[:, BAD] = skipped
    bad = np.argwhere(g != e)
    assert not len(bad), "%s: %s differs at %d places, first (step, pair) %s: got %s expected %s" % (where, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], e[tuple(bad[0])])


def views(dev):
    t, K = dev['torch'], dev['v'].n_items
    W = 2 * VIEW + 1
    bufs = (filled(dev, (T + 1, PAD, W * W), t.int8, S32), filled(dev, (T + 1, PAD), t.int32, S32), filled(dev, (T + 1, PAD, K), t.int32, S32))
    return bufs, _cabi.TrajViews(VIEW, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), PAD)


def assert_views(bufs, e, where):
    """The three view buffers against the oracle's rows, zero rows for BAD and for the lanes past COUNT (a wave stores whole tiles)."""
    spec, o, _, _ = twin()
    exp = VO.expect_views(spec, o.st, inputs()[0], e, VIEW)
    W = 2 * VIEW + 1
    for buf, k in zip(bufs, ('agent_map', 'agent_facing_id', 'inventory_items_quantity')):
        g, x = buf.cpu().numpy(), exp[k].reshape(T + 1, COUNT, -1).copy()
        x[:, BAD] = 0
        g = g.reshape(T + 1, PAD, -1)
        assert (g[:, :COUNT] == x).all() and (g[:, COUNT:] == 0).all(), (where, k, W)


def assert_kept(dev, ends, where):
    """The children of every pair but BAD are the oracle's end rows; BAD's slot is the never-saved row it was."""
    good = np.arange(COUNT) != BAD
    st = dev['pool'].state()
    RO.assert_rows(st, {k: np.asarray(x)[good] for k, x in ends.items()}, where, idx=np.arange(N, N + COUNT)[good])
    assert not np.asarray(st['map'])[N + BAD].any() and not np.asarray(st['inv'])[N + BAD].any(), "%s: the skipped pair's slot was written" % where


# ---------------------------------------------------------------- rollouts: the plan is read
@pytest.mark.gpu
def test_rollout_plain_skipped_pair_untouched_and_invalid_id_only_while_alive(dev):
    spec, o, _, _ = twin()
    po, plans, _, (live, lt), (over, ot), _ = inputs()
    L, t = dev['L'], dev['torch']
    only_over = plans.copy()
    only_over[lt, live] = 0
    for name, pl, want in (('an id outside the list in an ENDED pair', only_over, F_BAD_INDEX), ('and one in a LIVE pair', plans, F_BAD_INDEX | F_INVALID_ACTION)):
        ends, rep, alive = RO.oracle_slot_rollout(spec, o.st, po, pl.T, True, HORIZON)
        assert not alive[ot, over] and (pl is only_over or alive[lt, live]) and (rep['length'] < T).all() and (rep['length'] == 5).any()
        r, acts = reports(dev), dev['up'](pl)
        _cabi.check(L.ngw_snapshot_rollout(dev['v']._h, dev['pool']._s, ptr(dev['parents']), ptr(acts), COUNT, T, dev['pool']._s, ptr(dev['kids']), COUNT, *map(ptr, r)))
        # contract: F_INVALID_ACTION only while the pair is alive; the no-op step counts in `length` (the oracle's rule)
        assert flags_after(dev) == want, name
        # contract: a rollout leaves the four reports of a skipped pair untouched
        assert_reports(r, rep, 'untouched', name)
        assert_kept(dev, ends, name)


@pytest.mark.gpu
def test_rollout_path_and_traj_limits_keys_rewards_views_and_their_tail_fill(dev):
    spec, o, _, _ = twin()
    po, plans, limits, _, _, _ = inputs()
    L, t = dev['L'], dev['torch']
    e = TO.oracle_traj(spec, o.st, po, plans, limits, True, HORIZON, KEY_STATE)
    length = e['reports']['length']
    # the shape's conditions: the second wave stops at step 2 at the latest, no pair runs step 5, some pair runs step 4
    assert (length[64:] <= 2).all() and (length < T).all() and (length == 5).any() and (e['keys'][2:, 64:] == 0).all() and (e['keys'][5] == 0).all()
    acts, lim = dev['up'](plans), dev['up'](limits)
    # PATH: keys
    r, keys = reports(dev), filled(dev, (T, COUNT), t.int64, S64)
    _cabi.check(L.ngw_snapshot_rollout_path(dev['v']._h, dev['pool']._s, ptr(dev['parents']), ptr(acts), COUNT, T, ptr(lim), None, None, COUNT, *map(ptr, r), KEY_STATE,
                                            ptr(keys), COUNT))
    assert flags_after(dev) == F_BAD_INDEX | F_INVALID_ACTION
    assert_reports(r, e['reports'], 'untouched', 'rollout path')
    per_step(keys, e['keys'], 'rollout path', 'keys', 0)           # contract: keys 0 behind the limit, the end and the early exit - and for a skipped pair
    # TRAJ: rewards + views
    r, rew = reports(dev), filled(dev, (T, COUNT), t.int32, S32)
    bufs, vw = views(dev)
    _cabi.check(L.ngw_snapshot_rollout_traj_views(dev['v']._h, dev['pool']._s, ptr(dev['parents']), ptr(acts), COUNT, T, ptr(lim), None, None, COUNT, *map(ptr, r),
                                                  KEY_STATE, None, 0, ptr(rew), COUNT, None, 0, C.byref(vw)))
    assert flags_after(dev) == F_BAD_INDEX | F_INVALID_ACTION
    assert_reports(r, e['reports'], 'untouched', 'rollout traj')
    per_step(rew, e['rewards'], 'rollout traj', 'rewards', 0)      # contract: rewards 0 likewise
    assert_views(bufs, e, 'rollout traj')                          # contract: zero rows / views likewise


# ---------------------------------------------------------------- playouts: the actions are drawn
@pytest.mark.gpu
@pytest.mark.parametrize('weighted', [False, True], ids=['UNIFORM', 'WEIGHTED'])
def test_playout_path_and_traj_prefix_rule_philox_counter_and_stored_zeros(dev, weighted):
    spec, o, _, _ = twin()
    po, _, limits, _, _, weights = inputs()
    L, t = dev['L'], dev['torch']
    if weighted:
        ends, rep, actions, _ = SO.oracle_weighted_playout(spec, o.st, po, T, SEED, weights, FIRST_PAIR, True, HORIZON)
    else:
        ends, rep, actions, _ = PO.oracle_playout(spec, o.st, po, T, SEED, FIRST_PAIR, True, HORIZON)
    # contract: the Philox counter is (s >> 2, 0, lo32(p), hi32(p)) - the oracle's word; p crosses 2^32 inside the call and step 4 opens a second block
    assert FIRST_PAIR + COUNT > 1 << 32 and (actions[4] >= 0).any() and (rep['length'] < T).all()
    wt = dev['up'](weights) if weighted else None          # (held until the last call: the pointer alone does not keep the tensor)
    w = ptr(wt)
    # the unlimited playout, plain entry points: reports and recorded actions; a skipped pair's reports are STORED as 0, its actions as -1
    r, first, rec = reports(dev), filled(dev, (COUNT,), t.int32, S32), filled(dev, (T, COUNT), t.int32, S32)
    if weighted:
        rc = L.ngw_snapshot_playout_weighted(dev['v']._h, dev['pool']._s, ptr(dev['parents']), COUNT, T, SEED, FIRST_PAIR, w, dev['pool']._s, ptr(dev['kids']),
                                             *map(ptr, r), ptr(first), ptr(rec), COUNT)
    else:
        rc = L.ngw_snapshot_playout(dev['v']._h, dev['pool']._s, ptr(dev['parents']), COUNT, T, SEED, FIRST_PAIR, dev['pool']._s, ptr(dev['kids']), *map(ptr, r),
                                    ptr(first), ptr(rec), COUNT)
    _cabi.check(rc)
    assert flags_after(dev) == F_BAD_INDEX
    assert_reports(r, rep, 'zeros', 'playout')
    per_step(rec, actions, 'playout', 'actions', -1)               # contract: actions -1 for the steps no pair ran and for a skipped pair
    f = first.cpu().numpy()
    assert f[BAD] == -1 and (np.delete(f, BAD) == np.delete(actions[0], BAD)).all()
    assert_kept(dev, ends, 'playout')
    # contract: the limit folds into `alive` before the action is used - a limited playout is the prefix of the unlimited one, -1 beyond the limit
    e = TO.oracle_traj(spec, o.st, po, actions, limits, True, HORIZON, KEY_STATE)
    length = e['reports']['length']
    assert (length[64:] <= 2).all() and (length == np.minimum(rep['length'], np.clip(limits, 0, T))).all()
    cut = np.where(np.arange(T)[:, None] < length[None, :], actions, -1)
    lim = dev['up'](limits)
    r, first, rec, keys = reports(dev), filled(dev, (COUNT,), t.int32, S32), filled(dev, (T, COUNT), t.int32, S32), filled(dev, (T, COUNT), t.int64, S64)
    _cabi.check(L.ngw_snapshot_playout_path(dev['v']._h, dev['pool']._s, ptr(dev['parents']), COUNT, T, SEED, FIRST_PAIR, w, ptr(lim), None, None, *map(ptr, r),
                                            ptr(first), ptr(rec), COUNT, KEY_STATE, ptr(keys), COUNT))
    assert flags_after(dev) == F_BAD_INDEX
    assert_reports(r, e['reports'], 'zeros', 'playout path')
    per_step(rec, cut, 'playout path', 'actions', -1)
    per_step(keys, e['keys'], 'playout path', 'keys', 0)
    f = first.cpu().numpy()
    assert f[BAD] == -1 and (np.delete(f, BAD) == np.delete(cut[0], BAD)).all()      # (a pair limited to 0 steps: -1)
    # TRAJ: masks + views, every tail fill
    r, first, msk = reports(dev), filled(dev, (COUNT,), t.int32, S32), filled(dev, (T, COUNT), t.int64, S64)
    bufs, vw = views(dev)
    _cabi.check(L.ngw_snapshot_playout_traj_views(dev['v']._h, dev['pool']._s, ptr(dev['parents']), COUNT, T, SEED, FIRST_PAIR, w, ptr(lim), None, None, *map(ptr, r),
                                                  ptr(first), None, 0, KEY_STATE, None, 0, None, 0, ptr(msk), COUNT, None, 0, C.byref(vw)))
    assert flags_after(dev) == F_BAD_INDEX
    assert_reports(r, e['reports'], 'zeros', 'playout traj')
    per_step(msk, e['masks'], 'playout traj', 'masks', 0)          # contract: masks 0 for every step that did not run
    assert_views(bufs, e, 'playout traj')


@pytest.mark.gpu
def test_guided_stop_only_alive_lanes_walk_and_bad_weight_only_for_a_step_that_ran(dev):
    spec, o, _, _ = twin()
    po, _, limits, _, _, _ = inputs()
    L, t, v = dev['L'], dev['torch'], dev['v']
    A, craft = len(spec.actions_id), GO.craft_ids(spec)
    # the table: the parents' keys and the even steps' path keys of a plain playout under another seed (guided_playout_oracle.inputs' recipe)
    _, _, acts, _ = PO.oracle_playout(spec, o.st, po, T, FILL_SEED, 0, True, HORIZON)
    keys = KO.oracle_path(spec, o.st, po, acts, None, True, HORIZON, KEY_STATE)[0]
    own = keys_of_rows(RO._rows_of(XO.rows_state(spec, o.st, po)), KEY_STATE)
    members = np.array(list(dict.fromkeys(k for k in np.concatenate([own, keys[0::2].reshape(-1)]).tolist() if k)), np.uint64)
    table = v.key_table(len(members))
    found = table.insert(members)
    where_of = dict(zip(members.tolist(), np.asarray(found.where).tolist()))
    tw = dev['up'](GO.rows_for(members, found.where, table.buckets, A, craft))
    e = GO.oracle_guided(spec, o.st, po, T, SEED, members, lambda k: GO.row_of(k, A, craft), None, FIRST_PAIR, True, HORIZON, KEY_STATE, limits, True)
    length = e['reports']['length']
    assert not e['bad'] and e['events']['hits'] > 0 and ((length < np.clip(limits, 0, T)) & ~e['reports']['ended']).any(), "no pair is stopped by the table"
    # the default weights hold a NaN: with `stop` a lane that misses is no longer alive when its (default) row is read, so no step that ran reads it
    poison = dev['up'](np.full(A, np.nan, np.float32))
    lim = dev['up'](limits)
    r, first, rec = reports(dev), filled(dev, (COUNT,), t.int32, S32), filled(dev, (T, COUNT), t.int32, S32)
    where, depth, msk = filled(dev, (T, COUNT), t.int32, S32), filled(dev, (COUNT,), t.int32, S32), filled(dev, (T, COUNT), t.int64, S64)
    _cabi.check(L.ngw_snapshot_playout_guided(v._h, dev['pool']._s, ptr(dev['parents']), COUNT, T, SEED, FIRST_PAIR, ptr(poison), ptr(lim), None, None, *map(ptr, r),
                                              ptr(first), ptr(rec), COUNT, KEY_STATE, None, 0, None, 0, ptr(msk), COUNT, None, 0, None, table._open(), ptr(tw), ptr(where),
                                              COUNT, ptr(depth), 1))
    got = flags_after(dev)
    assert not got & F_BAD_WEIGHT, "F_BAD_WEIGHT raised by a lane whose step did not run"
    assert got == F_BAD_INDEX
    assert_reports(r, e['reports'], 'zeros', 'guided stop')
    per_step(rec, e['actions'], 'guided stop', 'actions', -1)
    per_step(msk, e['masks'], 'guided stop', 'masks', 0)
    exp_where = np.full((T, COUNT), -1, np.int32)
    for s, j in np.argwhere(e['hit']):
        exp_where[s, j] = where_of[int(e['before'][s, j])]
    per_step(where, exp_where, 'guided stop', 'where', -1)         # contract: where -1 for the steps that did not run; only alive lanes look up
    dp = depth.cpu().numpy()
    assert dp[BAD] == 0 and (np.delete(dp, BAD) == np.delete(e['depth'], BAD)).all()
    table.close()
