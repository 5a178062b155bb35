"""Expected snapshot rollouts from the unmodified CPU oracle: pairs_oracle.step_pairs - the parents' rows stepped T times in two copies, one under
the handle's autoreset setting and horizon for the reports and the per-step `alive` mask, one that never resets for the end rows - with the
given plans as its actions.  A step with an action id outside the list is a no-op in both copies: reward 0, info 0, it counts in `length`.
Nothing here comes from the HIP path (tests/test_slot_rollout*.py compare the device's end states and reports with these)."""
import numpy as np

import expand_oracle as XO
import ngw_testlib as T
import pairs_oracle as PA

STATE_KEYS = XO.STATE_KEYS
_rows_of, _step_rows = PA.rows_of, PA.step_rows


def oracle_slot_rollout(spec, rows, parents, plans, autoreset=False, horizon=0):
    """plans: integer [count, T], pair-major.  -> (ends, reports, alive): ends = {key: [count, ...]} the seven arrays of the rows as the last
    executed step leaves them, reports = {'ret' int32, 'length' int32, 'ended' bool, 'info' uint32}, each [count], alive = bool [T, count]:
    pair j executed step t.  `rows` is untouched."""
    plans = np.asarray(plans, np.int64)
    count, steps = plans.shape
    assert len(parents) == count and steps >= 1
    e = PA.step_pairs(spec, rows, parents, steps, plans.T, None, autoreset, horizon)
    return e['ends'], e['reports'], e['ran']


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
        rows, n_parents, own = self._source('rollout', from_envs, source)
        env = self.env
        a = check_plan_ids(plans, len(env.spec.actions_id))
        p, c, count = check_rollout(parents, int(a.shape[0]), children, n_parents, self.capacity, own)
        p = np.arange(count) if p is None else p
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
