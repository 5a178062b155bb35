"""Expected snapshot rollouts from the unmodified CPU oracle.  The parent rows are gathered into oracle States (expand_oracle.rows_state) and
stepped T times in two copies:
  - one under the handle's autoreset setting and horizon: its outputs are the expected reports - the info words assembled as
    tests/plan_oracle.py does - and its `done` gives the per-step `alive` mask (a pair stops at the first step whose done is set; that
    step counts);
  - one with autoreset off that only ever steps the pairs still alive: its rows are the expected end states, no reset ever runs on it,
    and an ended pair is frozen in the state it ended in.
A step with an action id outside the list is a no-op in both copies: reward 0, info 0, it counts in `length`.  Nothing here comes from the
HIP path (tests/test_slot_rollout*.py compare the device's end states and reports with these)."""
import numpy as np

import expand_oracle as XO
import ngw_testlib as T
from oracle.ngw_oracle import Oracle

STATE_KEYS = XO.STATE_KEYS


def _rows_of(st):
    return {k: getattr(st, k).copy() for k in STATE_KEYS}


def _step_rows(spec, cs, rows, idx, acts, autoreset, horizon):
    """Rows idx of `rows` stepped once with acts (one per index) in a fresh oracle; the stepped rows are written back.  -> the oracle."""
    o = Oracle(cs, len(idx), autoreset=autoreset, horizon=horizon)
    o.st = XO.rows_state(spec, rows, idx)
    o.step(np.ascontiguousarray(acts, np.int32))
    for k in STATE_KEYS:
        rows[k][idx] = getattr(o.st, k)
    return o


def oracle_slot_rollout(spec, rows, parents, plans, autoreset=False, horizon=0):
    """plans: integer [count, T], pair-major.  -> (ends, reports, alive): ends = {key: [count, ...]} the seven arrays of the rows as the last
    executed step leaves them, reports = {'ret' int32, 'length' int32, 'ended' bool, 'info' uint32}, each [count], alive = bool [T, count]:
    pair j executed step t.  `rows` is untouched."""
    cs = spec.compile()
    parents, plans = np.asarray(parents, np.int64), np.asarray(plans, np.int64)
    count, steps = plans.shape
    assert len(parents) == count and steps >= 1
    valid = (plans >= 0) & (plans < cs.n_actions)
    parent = XO.rows_state(spec, rows, parents)
    live_rows, end_rows = _rows_of(parent), _rows_of(parent)    # the copy under the handle's settings / the copy that never resets
    ret, length = np.zeros(count, np.int32), np.zeros(count, np.int32)
    ended, info = np.zeros(count, bool), np.zeros(count, np.uint32)
    alive, alive_at = np.ones(count, bool), np.zeros((steps, count), bool)
    for t in range(steps):
        if not alive.any():
            break
        alive_at[t] = alive
        length[alive] += 1
        info[alive] = 0                                         # (an invalid id: info word 0, reward 0)
        idx = np.nonzero(alive & valid[:, t])[0]
        if idx.size:
            r = _step_rows(spec, cs, live_rows, idx, plans[idx, t], autoreset, horizon)
            goal_done = (r.info >> np.uint32(1)) & np.uint32(1)
            word = (r.result.astype(np.uint32) | (goal_done << np.uint32(1)) | (r.cost_code.astype(np.uint32) << np.uint32(2)) |
                    (r.msg_code.astype(np.uint32) << np.uint32(8)) | (r.msg_arg.astype(np.uint32) << np.uint32(16)))
            ret[idx] += r.reward
            info[idx] = word
            _step_rows(spec, cs, end_rows, idx, plans[idx, t], False, 0)
            done = r.done.astype(bool)
            ended[idx[done]] = True
            alive[idx[done]] = False
    ends = {k: end_rows[k].astype(getattr(parent, k).dtype) for k in STATE_KEYS}
    assert (ends['episode'] == parent.episode).all()
    return ends, dict(ret=ret, length=length, ended=ended, info=info), alive_at


def assert_reports(got, exp, where):
    """ret / length / ended / info of `got` (a PlanEval of numpy arrays) equal the oracle's; names the first pair that differs."""
    for k in ('ret', 'length', 'ended', 'info'):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if k == 'info' and g.dtype.kind == 'i':
            g = g.astype(np.int64).astype(np.uint32)
        assert g.shape == e.shape, "%s: %s shape %r expected %r" % (where, k, g.shape, e.shape)
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, "%s: %s differs in %d pairs, first pair %d: got %r expected %r (info got %#x expected %#x)" % (
            where, k, bad.size, bad[0], g[bad[0]], e[bad[0]], int(np.asarray(got['info'])[bad[0]]) & 0xFFFFFFFF, int(exp['info'][bad[0]]))


assert_rows = XO.assert_rows


class _BoundRolloutSnapshot(XO._BoundExpandSnapshot):
    """expand_oracle's bound snapshot with Snapshot.rollout: the product's host checks (snapshot.check_plan_ids, check_rollout), the
    oracle's steps."""

    def rollout(self, parents, plans, children=None, from_envs=False, source=None, device=False):
        from gym_novel_gridworlds_amd.snapshot import check_plan_ids, check_rollout
        from gym_novel_gridworlds_amd.vec_env import PlanEval
        self._open()
        if source is not None and from_envs:
            raise ValueError("rollout: give either source or from_envs")
        src = self if source is None else source
        if not from_envs:
            if not isinstance(src, XO._BoundExpandSnapshot):
                raise ValueError("source: a Snapshot expected")
            src._open()
            if src.env is not self.env:
                raise ValueError("source: a snapshot of another env")
        env = self.env
        n_parents = env.num_envs if from_envs else src.capacity
        a = check_plan_ids(plans, len(env.spec.actions_id))
        p, c, count = check_rollout(parents, int(a.shape[0]), children, n_parents, self.capacity, not from_envs and src is self)
        p = np.arange(count) if p is None else p
        rows = env.o.st if from_envs else src.model.rows
        ends, rep, _ = oracle_slot_rollout(env.spec, rows, p, a, env.o.autoreset, env.o.horizon)
        if c is not None:
            for k in STATE_KEYS:
                self.model.rows[k][c] = ends[k]
        return PlanEval(rep['ret'], rep['length'], rep['ended'], rep['info'])


class OracleVecRollout(XO.OracleVecExpand):
    """expand_oracle.OracleVecExpand whose snapshots roll out: lets the host logic run without a GPU."""

    def snapshot(self, capacity=None):
        s = _BoundRolloutSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s


__all__ = ['T', 'oracle_slot_rollout', 'assert_reports', 'assert_rows', 'OracleVecRollout', 'STATE_KEYS']
