"""Expected path keys from the unmodified CPU oracle.  The recorded (or given) actions of every pair are replayed from a host copy of the parents'
rows by slot_rollout_oracle's helpers - one copy under the handle's autoreset setting and horizon for the reports and the `alive` mask, one
that never resets for the rows - and the key of the state after every executed step is state_keys.keys_of_rows of those rows (the host
statement of the key contract).  Nothing here uses the device's own step, mask or key (tests/test_path_keys*.py compare the HIP path with
these)."""
import numpy as np

import expand_oracle as XO
import sample_oracle as SO
import slot_rollout_oracle as RO
from gym_novel_gridworlds_amd.state_keys import KEY_STATE, keys_of_rows

STATE_KEYS = RO.STATE_KEYS


def oracle_path(spec, rows, parents, actions, limits=None, autoreset=False, horizon=0, fields=KEY_STATE):
    """actions: integer [T, count], step-major (what playout(record=True) returns and rollout() takes as a device tensor); an id outside the
    action list is a no-op step that counts.  limits: None or [count] integers, clamped to [0, T].
    -> (keys uint64 [T, count] - 0 for a step the pair did not execute -, reports {'ret', 'length', 'ended', 'info'}, ends: the rows as the last
    executed step leaves them, states: {(t, j): the row after step t of pair j, a dict of the seven arrays}, events: a dict of counts the
    tests use to show that their inputs met what they are about)."""
    cs = spec.compile()
    parents, actions = np.asarray(parents, np.int64), np.asarray(actions, np.int64)
    steps, count = actions.shape
    lim = np.full(count, steps, np.int64) if limits is None else np.clip(np.asarray(limits, np.int64), 0, steps)
    valid = (actions >= 0) & (actions < cs.n_actions)
    parent = XO.rows_state(spec, rows, parents)
    live_rows, end_rows = RO._rows_of(parent), RO._rows_of(parent)
    ret, length = np.zeros(count, np.int32), np.zeros(count, np.int32)
    ended, info = np.zeros(count, bool), np.zeros(count, np.uint32)
    keys, states = np.zeros((steps, count), np.uint64), {}
    ev = dict(pickups=0, inv_jumps=0, deaths=0, cuts=0, limited=0, map_writes=0, double_counts=0)
    alive = np.ones(count, bool)
    for t in range(steps):
        ev['limited'] += int((alive & (lim <= t)).sum())
        alive &= lim > t
        if not alive.any():
            break
        length[alive] += 1
        info[alive] = 0
        idx = np.nonzero(alive & valid[t])[0]
        if idx.size:
            before_map, before_inv, before_loc = end_rows['map'][idx].copy(), end_rows['inv'][idx].copy(), end_rows['loc'][idx].copy()
            before_steps = end_rows['step_count'][idx].copy()
            r = RO._step_rows(spec, cs, live_rows, idx, actions[t, idx], autoreset, horizon)
            goal_done = (r.info >> np.uint32(1)) & np.uint32(1)
            info[idx] = (r.result.astype(np.uint32) | (goal_done << np.uint32(1)) | (r.cost_code.astype(np.uint32) << np.uint32(2)) |
                         (r.msg_code.astype(np.uint32) << np.uint32(8)) | (r.msg_arg.astype(np.uint32) << np.uint32(16)))
            ret[idx] += r.reward
            RO._step_rows(spec, cs, end_rows, idx, actions[t, idx], False, 0)
            done = r.done.astype(bool)
            ended[idx[done]] = True
            alive[idx[done]] = False
            n = len(idx)
            cells = (before_map.reshape(n, -1) != end_rows['map'][idx].reshape(n, -1)).sum(1)
            moved = (before_loc != end_rows['loc'][idx]).any(1)
            ev['map_writes'] += int((cells > 0).sum())
            ev['pickups'] += int(((cells > 0) & moved).sum())                  # a cell changed by a step that moved the agent: an entity picked up
            ev['inv_jumps'] += int(((before_inv != end_rows['inv'][idx]).sum(1) >= 2).sum())   # two or more entries at once: a crate opened, a craft
            ev['double_counts'] += int((end_rows['step_count'][idx] - before_steps == 2).sum())   # FenceRestriction's second count
            ev['deaths'] += int((done & (r.msg_code == 14)).sum())
            ev['cuts'] += int((done & (goal_done == 0) & (r.msg_code != 14)).sum())
        ran = np.nonzero(lim > t)[0]
        ran = ran[length[ran] == t + 1]                                        # the pairs that executed step t (a no-op id included)
        if ran.size:
            now = {k: end_rows[k][ran] for k in STATE_KEYS}
            keys[t, ran] = keys_of_rows(now, fields)
            for i, j in enumerate(ran):
                states[(t, int(j))] = {k: now[k][i].copy() for k in STATE_KEYS}
    ends = {k: end_rows[k].astype(getattr(parent, k).dtype) for k in STATE_KEYS}
    return keys, dict(ret=ret, length=length, ended=ended, info=info), ends, states, ev


def assert_keys(got, exp, where):
    g = np.asarray(got)
    if g.dtype.kind == 'i':
        g = g.view(np.uint64)
    assert g.shape == exp.shape and g.dtype == np.uint64, (where, g.shape, g.dtype, exp.shape)
    bad = np.argwhere(g != exp)
    assert not len(bad), "%s: keys differ at %d of %d places, first (step, pair) %s: got %#x expected %#x" % (
        where, len(bad), g.size, tuple(bad[0]), int(g[tuple(bad[0])]), int(exp[tuple(bad[0])]))


class OracleVecPath(SO.OracleVecSample):
    """sample_oracle.OracleVecSample whose playouts() take path_keys / fields: lets the adapter's, the wrappers' and the sharded env's
    forwarding run without a GPU."""

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, path_keys=False, fields=None):
        from gym_novel_gridworlds_amd.playout import Playout, PlayoutPath
        P, N = int(n_playouts), self.num_envs
        parents = np.repeat(np.arange(N), P)
        if weights is None:
            _, rep, acts, _ = SO.PO.oracle_playout(self.spec, self.o.st, parents, steps, seed, self.env_index_base * P, self.o.autoreset, self.o.horizon)
        else:
            _, rep, acts, _ = SO.oracle_weighted_playout(self.spec, self.o.st, parents, steps, seed, weights, self.env_index_base * P, self.o.autoreset,
                                                         self.o.horizon)
        play = Playout(rep['ret'], rep['length'], rep['ended'], rep['info'], rep['first_action'], None)
        if not path_keys:
            return play.shaped(N, P)
        keys, _, _, _, _ = oracle_path(self.spec, self.o.st, parents, acts, None, self.o.autoreset, self.o.horizon, KEY_STATE if fields is None else fields)
        return PlayoutPath(*play, keys).shaped(N, P)


def sharded_on_oracle(**kw):
    """The product's ShardedVecNovelGridworld with its local env replaced by OracleVecPath (no GPU)."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld

    class OracleSharded(ShardedVecNovelGridworld):
        def _make_local(self, device=None, spec=None, **k):
            k = {a: b for a, b in k.items() if a in ('num_envs', 'seed', 'autoreset', 'horizon', 'env_index_base')}
            return OracleVecPath(spec, **k)

    return OracleSharded(**kw)
