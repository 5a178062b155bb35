"""Guided playouts on the MI355X (playout(table=, table_weights=, outside=): csrc/ngw_playout.inc GUIDED, csrc/ngw_table.inc table_find, include/ngw.h
ngw_snapshot_playout_guided), held to the CPU forward simulation of tests/guided_playout_oracle.py - the oracle's steps, masks and keys and the public
numpy contracts of the Philox word and the weighted choice; never the device's own.  Everything is an integer and compared bit for bit.

Shapes: 130 pairs (two full waves and two lanes) with repeated parents, T = 12.  Configurations: pogo10; axe11 (S * S = 121, pick-ups, 18 actions);
fire12h (FireWall hard 12 x 12, autoreset with a horizon, KEY_STEP_COUNT in the key); pogo10lim (the action table LimitActions' playouts run on).
The table holds the parents' keys and the even steps' path keys of a plain playout under another seed, capacity = the number of distinct keys; row
where_of(key) of table_weights is f(key): peaked rows, all-zero rows, rows with weight on crafting actions only.  The coverage conditions of the
outside='default' parity cases (>= 20 % hits, >= 20 % misses, a re-entry, a zero-mass row read, a hit step whose action differs from the default's, a key
outside its home bucket) are asserted here under the oracle alone and in test_guided_playout_cpu.py for the same seeds."""

import numpy as np
import pytest

import guided_playout_oracle as GO
import path_key_oracle as KO
import slot_observe_oracle as OO
import slot_rollout_oracle as RO
import trajectory_oracle as TO
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.playout import PlayoutGuided, tree_steps
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX

pytestmark = pytest.mark.gpu
F_BAD_WEIGHT = 16
COUNT, STEPS, SEED = GO.COUNT, GO.STEPS, GO.SEED


def make(name, lidar=False):
    """The device twin of GO.twin(name), its table filled with the member keys, and the weight rows -> (spec, env, pool, table, where_of, tw)."""
    spec, o, seed, kw, warmup = GO.twin(name)
    v = VecNovelGridworld(spec=spec, num_envs=GO.N, seed=seed, **kw)
    v.reset()
    for a in warmup:
        v.step(a)
    if kw:
        v.set_state(0, step_count=np.asarray(o.st.step_count, np.int32))
    if lidar:
        v.lidar_configure(GO.lidar_cfg(name), dtype=np.int32)
    _, _, members = GO.inputs(name)
    table = v.key_table(len(members))
    found = table.insert(members)
    assert found.fresh.all() and (found.where >= 0).all() and len(table) == len(members)
    A = len(spec.actions_id)
    tw = GO.rows_for(members, found.where, table.buckets, A, GO.craft_ids(spec))
    pool = v.snapshot(GO.N + COUNT)
    pool.save()
    return spec, v, pool, table, dict(zip(members.tolist(), found.where.tolist())), tw


def expect_where(e, where_of):
    w = np.full(e['hit'].shape, -1, np.int32)
    for t, j in np.argwhere(e['hit']):
        w[t, j] = where_of[int(e['before'][t, j])]
    return w


def assert_guided(got, e, where_of, where, fields=('rewards', 'masks')):
    assert isinstance(got, PlayoutGuided), type(got)
    if hasattr(got.ret, 'data_ptr'):
        got = type(got)(*[None if x is None else OO.host(x) for x in got])._replace(info=OO.host(got.info).view(np.uint32))
    RO.assert_reports(got, e['reports'], where)
    if got.actions is not None:
        bad = np.argwhere(got.actions != e['actions'])
        assert not len(bad), "%s: actions differ at %d places, first (step, pair) %s" % (where, len(bad), tuple(bad[0]))
    assert (got.first_action == e['actions'][0]).all(), where
    exp_w = expect_where(e, where_of)
    assert got.where.dtype == np.int32 and got.where.shape == exp_w.shape, (where, got.where.dtype, got.where.shape)
    bad = np.argwhere(got.where != exp_w)
    assert not len(bad), "%s: where differs at %d places, first (step, pair) %s: got %d expected %d" % (
        where, len(bad), tuple(bad[0]), got.where[tuple(bad[0])], exp_w[tuple(bad[0])])
    assert got.depth.dtype == np.int32 and (got.depth == e['depth']).all(), where
    TO.assert_traj(got, e, where, [k for k in fields if getattr(got, k, None) is not None])
    if got.keys is not None:
        KO.assert_keys(got.keys, e['keys'], where)


@pytest.mark.parametrize('name', list(GO.CONFIGS))
def test_against_the_oracle(name):
    """Full parity of both `outside` rules: actions, where, depth, reports, keys, rewards, masks, and the kept children."""
    e = GO.expected(name)
    GO.coverage(e)
    spec, v, pool, table, where_of, tw = make(name)
    parents, default, members = GO.inputs(name)
    assert (GO.home_buckets(members, table.buckets) != np.array([where_of[k] for k in members.tolist()])).any(), "no probe chain: every key sits at home"
    _, _, _, fields, _ = GO.CONFIGS[name]
    kids = np.arange(GO.N, GO.N + COUNT)
    got = pool.playout(parents, STEPS, SEED, children=kids, record=True, weights=default, path_keys=True, fields=fields, rewards=True, masks=True, table=table,
                       table_weights=tw)
    assert_guided(got, e, where_of, name)
    RO.assert_rows(pool.state(), e['ends'], name, idx=kids)
    assert (got.where >= 0).sum() == e['events']['hits'] and ((got.where < 0) & (got.actions >= 0)).sum() == e['events']['misses']
    b, a, t, j = tree_steps(got)
    assert len(b) == e['events']['hits'] and (got.where[t, j] == b).all() and (got.actions[t, j] == a).all()
    assert v.error_flags() == 0
    # outside='stop': lengths, `ended`, the kept children, and the last key being the absent state's
    s = GO.expected(name, stop=True)
    stop = pool.playout(parents, STEPS, SEED, children=kids, record=True, weights=default, path_keys=True, fields=fields, rewards=True, masks=True, table=table,
                        table_weights=tw, outside='stop', device=True)
    assert_guided(stop, s, where_of, name + ' stop')
    RO.assert_rows(pool.state(), s['ends'], name + ' stop', idx=kids)
    length, keys = s['reports']['length'], OO.host(stop.keys).view(np.uint64)
    cut = np.nonzero(~s['reports']['ended'] & (length < STEPS) & (length > 0))[0]
    assert cut.size > 0 and not set(keys[length[cut] - 1, cut].tolist()) & set(members.tolist()), "a pair cut by the table stops in a state the table does not hold"
    assert (OO.host(stop.where)[OO.host(stop.actions) >= 0] >= 0).all() and (OO.host(stop.depth) == length).all()
    # nothing is committed: the env, the table's count and every member's bucket
    assert len(table) == len(members) and (table.lookup(members) == np.array([where_of[k] for k in members.tolist()])).all()
    st, ost = v.get_state(), GO.twin(name)[1].st
    assert (st['map'].reshape(GO.N, -1) == np.asarray(ost.map).reshape(GO.N, -1)).all() and (st['inv'] == ost.inv).all() and (st['step_count'] == ost.step_count).all()
    assert v.error_flags() == 0
    v.close()


def test_limits_stop_and_a_large_first_pair_from_envs_and_from_another_snapshot():
    """The smallest fixed shape of what tests/search_fuzz.py draws for a guided call, where a failure there can be moved to: fire12h (autoreset, a
    horizon, the step count in the key), 130 pairs, T = 12, limits drawn in [0, T] together with outside='stop', first_pair = 2^33 + 5, children
    kept - once from the live envs, once from another snapshot -, every field and the kept rows against the oracle."""
    name = 'fire12h'
    spec, v, pool, table, where_of, tw = make(name)
    parents, default, members = GO.inputs(name)
    _, o, _, _, _ = GO.twin(name)
    _, _, auto, fields, _ = GO.CONFIGS[name]
    assert auto and fields == GO.KEY_STATE | GO.KEY_STEP_COUNT
    A, craft, first_pair = len(spec.actions_id), GO.craft_ids(spec), 2 ** 33 + 5
    limits = np.random.RandomState(12).randint(0, STEPS + 1, COUNT).astype(np.int32)
    e = GO.oracle_guided(spec, o.st, parents, STEPS, SEED, members, lambda k: GO.row_of(k, A, craft), default, first_pair, True, GO.HORIZON, fields, limits, True)
    length, ended = e['reports']['length'], e['reports']['ended']
    assert (length == limits).any() and (~ended & (length < limits)).any() and ended.any(), "pairs cut by their limit, by the table and by their episode's end"
    assert (length == 0).any() and (length > 1).any() and (e['actions'] != GO.expected(name, stop=True)['actions']).any()
    kw = dict(record=True, weights=default, limits=limits, first_pair=first_pair, path_keys=True, fields=fields, rewards=True, masks=True, table=table,
              table_weights=tw, outside='stop')
    kids = np.arange(GO.N, GO.N + COUNT)
    got = pool.playout(parents, STEPS, SEED, children=kids, from_envs=True, **kw)
    assert_guided(got, e, where_of, 'from the envs')
    RO.assert_rows(pool.state(), e['ends'], 'from the envs', idx=kids)
    other = v.snapshot(COUNT)
    got = other.playout(parents, STEPS, SEED, children=np.arange(COUNT), source=pool, device=True, **kw)
    assert_guided(got, e, where_of, 'from another snapshot')
    RO.assert_rows(other.state(), e['ends'], 'from another snapshot', idx=np.arange(COUNT))
    RO.assert_rows(pool.state(), e['ends'], 'the source keeps its rows', idx=kids)
    assert len(table) == len(members) and v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('observe', ['lidar', 'agent_view'])
def test_observations_of_both_kinds(observe):
    name = 'axe11'
    lidar = observe == 'lidar'
    e = GO.expected(name, lidar=lidar)
    spec, v, pool, table, where_of, tw = make(name, lidar=lidar)
    parents, default, _ = GO.inputs(name)
    got = pool.playout(parents, STEPS, SEED, weights=default, rewards=True, observe=observe, view_size=2 if not lidar else 5, table=table, table_weights=tw)
    assert_guided(got, e, where_of, observe, ('rewards',))
    assert got.keys is None and got.actions is None
    if lidar:
        TO.assert_traj(got, e, observe, ('obs',))
    else:
        VO.assert_views(got.obs, VO.expect_views(spec, GO.twin(name)[1].st, parents, e, 2), observe)
    v.close()


def test_the_two_bit_identities_and_a_split_call():
    name = 'pogo10'
    spec, v, pool, table, where_of, tw = make(name)
    parents, default, members = GO.inputs(name)
    kw = dict(record=True, path_keys=True, rewards=True, masks=True, device=True)
    same = lambda a, b: all((x == y).all() for x, y in zip(a[:9], b[:9]))   # noqa: E731  (ret .. masks)
    empty = v.key_table(len(members))
    for weights in (None, default):
        plain = pool.playout(parents, STEPS, SEED, weights=weights, **kw)
        got = pool.playout(parents, STEPS, SEED, weights=weights, table=empty, table_weights=tw, **kw)
        assert same(got, plain) and (got.where == -1).all() and (got.depth == 0).all()
    A = len(spec.actions_id)
    every = np.ascontiguousarray(np.broadcast_to(default, (table.buckets, A)))
    import torch
    ref = pool.playout(parents, STEPS, SEED, weights=default, **kw)
    assert same(pool.playout(parents, STEPS, SEED, weights=default, table=table, table_weights=every, **kw), ref)
    # without default weights the misses draw uniformly: the pairs walk the weighted playout's path for as long as they stay inside the table
    got = pool.playout(parents, STEPS, SEED, table=table, table_weights=every, **kw)
    inside = torch.arange(STEPS, device=got.depth.device)[:, None] < got.depth[None, :]
    assert inside.any() and (got.actions[inside] == ref.actions[inside]).all() and (got.where[inside] >= 0).all() and not same(got, ref)
    # a call split with first_pair equals the whole call
    whole = pool.playout(parents, STEPS, SEED, weights=default, table=table, table_weights=tw, **kw)
    cut = 70
    a = pool.playout(parents[:cut], STEPS, SEED, weights=default, table=table, table_weights=tw, **kw)
    b = pool.playout(parents[cut:], STEPS, SEED, weights=default, table=table, table_weights=tw, first_pair=cut, **kw)
    for i, (x, y, z) in enumerate(zip(whole, a, b)):
        if x is not None:
            assert (torch.cat([y, z], -1 if x.dim() > 1 else 0) == x).all(), PlayoutGuided._fields[i]
    assert v.error_flags() == 0
    v.close()


def test_a_bad_index_and_bad_weights():
    import torch
    name = 'pogo10'
    e = GO.expected(name)
    spec, v, pool, table, where_of, tw = make(name)
    parents, default, members = GO.inputs(name)
    dev = torch.device('cuda:%d' % v.device)
    # F_BAD_WEIGHT only from a row that is read: NaN in every row no member owns raises nothing ...
    A = len(spec.actions_id)
    unread = GO.rows_for(members, [where_of[k] for k in members.tolist()], table.buckets, A, GO.craft_ids(spec), fill=np.nan)
    got = pool.playout(parents, STEPS, SEED, record=True, weights=default, table=table, table_weights=unread)
    assert (got.actions == e['actions']).all() and v.error_flags() == 0
    # ... a member row nobody visits raises nothing either, and one that is read does
    visited = set(e['before'][e['hit']].tolist())
    quiet = next(k for k in members.tolist() if k not in visited)
    row = tw.copy()
    row[where_of[quiet], 0] = -1.0
    pool.playout(parents, STEPS, SEED, weights=default, table=table, table_weights=row)
    assert v.error_flags() == 0
    row[where_of[int(e['before'][0, 0])], 1] = np.inf
    pool.playout(parents, STEPS, SEED, weights=default, table=table, table_weights=row)
    assert v.error_flags() == F_BAD_WEIGHT
    # a device index out of range: the pair is skipped, where -1, depth 0, F_BAD_INDEX 
    idx = torch.tensor(parents, dtype=torch.int32, device=dev)
    idx[5], idx[129] = 10 ** 6, -3
    got = pool.playout(idx, STEPS, SEED, record=True, weights=default, table=table, table_weights=tw)
    for j in (5, 129):
        assert (got.where[:, j] == -1).all() and got.depth[j] == 0 and (got.actions[:, j] == -1).all() and got.length[j] == 0
    ok = np.setdiff1d(np.arange(COUNT), [5, 129])
    assert (got.where[:, ok] == expect_where(e, where_of)[:, ok]).all() and (got.actions[:, ok] == e['actions'][:, ok]).all()
    assert v.error_flags() == F_BAD_INDEX                           # (reading the flags clears them: the weight flag was read above)
    v.close()


def test_playouts_and_the_adapter():
    import ngw_testlib as T
    name = 'pogo10'
    spec, v, pool, table, where_of, tw = make(name)
    _, default, members = GO.inputs(name)
    _, o, _, _, _ = GO.twin(name)
    P, A = 3, len(spec.actions_id)
    e = GO.oracle_guided(spec, o.st, np.repeat(np.arange(GO.N), P), STEPS, SEED, members, lambda k: GO.row_of(k, A, GO.craft_ids(spec)), default)
    got = v.playouts(P, STEPS, SEED, weights=default, path_keys=True, table=table, table_weights=tw)
    assert got.where.shape == (STEPS, GO.N, P) and got.depth.shape == (GO.N, P) and got.keys.shape == (STEPS, GO.N, P)
    flat = PlayoutGuided(*[None if x is None else (x.reshape(x.shape[0], -1) if x.ndim == 3 else x.reshape(-1)) for x in got])
    assert_guided(flat, e, where_of, 'playouts')
    v.close()
    env = T.make_adapter_env('pogo10')
    env.reset()
    for a in (0, 1, 0, 2):
        env.step(a)
    base = getattr(env, 'unwrapped', env)                           # (a plain configuration has no wrapper on the adapter)
    vec = base._backend()
    t2 = base.key_table(8)
    key = np.array([base.state_key()], np.uint64)
    b = int(t2.insert(key).where[0])
    w2 = np.zeros((t2.buckets, vec.n_actions), np.float32)
    first = int(np.flatnonzero(np.asarray(env.action_masks()))[-1])  # the root's row: all its weight on one valid action
    w2[b, first] = 1.0
    play = env.playouts(5, 4, SEED, table=t2, table_weights=w2)
    assert play.where.shape == (4, 5) and (play.where[0] == b).all() and (play.first_action == first).all() and (play.depth >= 1).all()
    env.close()


def test_limit_actions_on_the_adapter():
    """The LimitActions wrapper itself, with a permuted id table: the table is lim.key_table()'s (the limited env's), the columns of table_weights
    and the default weights are in the wrapper's id space - from the host and as a device tensor -, first_action comes back in it, and where /
    depth / keys are the oracle's under the limited action table."""
    import ngw_testlib as T
    import torch
    import expand_oracle as XO
    import playout_oracle as PO
    from gym_novel_gridworlds_amd.state_keys import KEY_STATE, keys_of_rows
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    env = T.make_adapter_env('axe10')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    rows = env.unwrapped._backend().get_state()
    wrapper_id = {'Break': 2, 'Forward': 0, 'Left': 3, 'Right': 1}
    names = sorted(wrapper_id)
    lim = LimitActions(env, set(names))
    lim.set_limited_actions_id(dict(wrapper_id))
    ids = [wrapper_id[n] for n in names]                            # the kernel's action i is the wrapper's ids[i]
    P, steps, A = 66, 8, len(names)
    zeros = np.zeros(P, np.int64)
    table = lim.key_table(256)
    limited = lim.__dict__['_playout_env'][2]
    lspec = limited.spec
    assert list(lspec.actions_id) == names and table.env is limited
    _, _, acts, _ = PO.oracle_playout(lspec, rows, zeros, steps, GO.FILL_SEED)
    path, _, _, _, _ = KO.oracle_path(lspec, rows, zeros, acts, None, False, 0, KEY_STATE)
    own = keys_of_rows(RO._rows_of(XO.rows_state(lspec, rows, zeros[:1])), KEY_STATE)
    members = np.unique(np.concatenate([own, path[0::2].reshape(-1)]))
    members = members[members != 0]
    found = table.insert(members)
    where_of = dict(zip(members.tolist(), found.where.tolist()))
    kernel_rows = GO.rows_for(members, found.where, table.buckets, A, [])
    default_k = np.array([0, 2, 1, 1], np.float32)
    tw, default = np.zeros_like(kernel_rows), np.zeros(A, np.float32)
    tw[:, ids], default[ids] = kernel_rows, default_k               # the wrapper's id space
    e = GO.oracle_guided(lspec, rows, zeros, steps, SEED, members, lambda k: GO.row_of(k, A, []), default_k)
    ev = e['events']
    assert ev['hits'] > 0 and ev['misses'] > 0 and ev['differs'] > 0 and ids != list(range(A))
    dev = torch.device('cuda:%d' % limited.device)
    results = [lim.playouts(P, steps, SEED, weights=default, path_keys=True, table=table, table_weights=x)
               for x in (tw, torch.from_numpy(tw).to(dev))]
    for got in results:
        assert isinstance(got, PlayoutGuided) and got.where.shape == (steps, P) and got.depth.shape == (P,)
        RO.assert_reports(got, e['reports'], 'LimitActions')
        assert (got.first_action == np.asarray(ids, np.int32)[e['actions'][0]]).all()
        assert (got.where == expect_where(e, where_of)).all() and (got.depth == e['depth']).all()
        KO.assert_keys(got.keys, e['keys'], 'LimitActions')
    assert limited.error_flags() == 0 and len(table) == len(members)
    lim.close()
