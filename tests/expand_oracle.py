"""Expected snapshot expansions from the unmodified CPU oracle: the parent rows are gathered into an oracle State, one copy is stepped with
autoreset off - its state after the step is the expected child, no reset ever runs on it -, another copy is stepped under the handle's
autoreset setting and horizon - its outputs are the expected reports, the info words assembled as tests/plan_oracle.py does.  A pair with
an action id outside the list expects the parent's row and zero reports.  Nothing here comes from the HIP path (tests/test_expand*.py
compare the device's children and reports with these)."""
import functools

import numpy as np

import mask_oracle as M
import ngw_testlib as T
import snapshot_oracle as SO
from oracle.ngw_oracle import Oracle

STATE_KEYS = SO.STATE_KEYS


def rows_state(spec, rows, idx):
    """An oracle State of len(idx) envs: rows idx of `rows` (a dict keyed as get_state() keys it, or an oracle State)."""
    get = (lambda k: rows[k]) if isinstance(rows, dict) else (lambda k: getattr(rows, k))
    idx = np.asarray(idx, np.int64)
    st = M.state_from(spec, get('map')[idx], get('loc')[idx], get('facing')[idx], get('inv')[idx], get('selected')[idx],
                      step_count=get('step_count')[idx])
    st.episode[...] = get('episode')[idx]
    return st


def oracle_expand(spec, rows, parents, actions, autoreset=False, horizon=0):
    """-> (children, reports): children = {key: [count, ...]} the seven arrays of the stepped rows, reports = {'reward' int32, 'done' bool,
    'result' bool, 'info' uint32}, each [count].  `rows` is untouched."""
    cs = spec.compile()
    parents, actions = np.asarray(parents, np.int64), np.asarray(actions, np.int64)
    count = len(parents)
    valid = (actions >= 0) & (actions < cs.n_actions)
    act = np.ascontiguousarray(np.where(valid, actions, 0), np.int32)
    parent = rows_state(spec, rows, parents)
    o = Oracle(cs, count, autoreset=False)                      # the child: the step's effects, never a reset
    o.st = parent.copy()
    o.step(act)
    children = {k: np.where(valid.reshape((-1,) + (1,) * (getattr(parent, k).ndim - 1)), getattr(o.st, k), getattr(parent, k)) for k in STATE_KEYS}
    children = {k: v.astype(getattr(parent, k).dtype) for k, v in children.items()}
    assert (children['episode'] == parent.episode).all()
    r = Oracle(cs, count, autoreset=autoreset, horizon=horizon)  # the reports: what the handle's own step would say
    r.st = parent.copy()
    r.step(act)
    reports = dict(reward=np.where(valid, r.reward, 0).astype(np.int32), done=r.done.astype(bool) & valid,
                   result=r.result.astype(bool) & valid, info=np.where(valid, T.info_word(r), 0).astype(np.uint32))
    return children, reports


def assert_rows(got, exp, where, idx=None):
    """The seven arrays of `got` (rows idx, default all) equal exp's; names the first row that differs."""
    for k in STATE_KEYS:
        g = np.asarray(got[k]) if idx is None else np.asarray(got[k])[np.asarray(idx)]
        e = np.asarray(exp[k])
        g = g.reshape(e.shape)
        bad = np.nonzero((g != e).reshape(len(e), -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs for %d rows, first pair %d: got %r expected %r" % (where, k, bad.size, bad[0], g[bad[0]], e[bad[0]])


def assert_reports(got, exp, where):
    for k in ('reward', 'done', 'result', 'info'):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if k == 'info':
            g = g.astype(np.int64).astype(np.uint32) if g.dtype.kind == 'i' else g
        assert g.shape == e.shape, "%s: %s shape %r expected %r" % (where, k, g.shape, e.shape)
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, "%s: %s differs in %d pairs, first pair %d: got %r expected %r (info got %#x expected %#x)" % (
            where, k, bad.size, bad[0], g[bad[0]], e[bad[0]], int(np.asarray(got['info'])[bad[0]]) & 0xFFFFFFFF, int(exp['info'][bad[0]]))


class _BoundExpandSnapshot(SO._BoundSnapshot):
    """snapshot_oracle's bound snapshot with Snapshot.expand / expand_all: the product's host checks (snapshot.check_expand,
    all_actions_pairs), the oracle's step."""

    def _source(self, call, from_envs, source):
        """The parents of a call: -> (their rows, how many there are, are they this snapshot's own slots)."""
        self._open()
        if source is not None and from_envs:
            raise ValueError("%s: give either source or from_envs" % call)
        if from_envs:
            return self.env.o.st, self.env.num_envs, False
        src = self if source is None else source
        if not isinstance(src, _BoundExpandSnapshot):
            raise ValueError("source: a Snapshot expected")
        src._open()
        if src.env is not self.env:
            raise ValueError("source: a snapshot of another env")
        return src.model.rows, src.capacity, src is self

    def expand(self, parents, actions, children, from_envs=False, source=None, device=False):
        from gym_novel_gridworlds_amd.snapshot import Expansion, check_expand
        rows, n_parents, own = self._source('expand', from_envs, source)
        env = self.env
        p, a, c, count = check_expand(parents, actions, children, n_parents, self.capacity, len(env.spec.actions_id), own)
        p = np.arange(count) if p is None else p
        c = np.arange(count) if c is None else c
        kids, rep = oracle_expand(env.spec, rows, p, a, env.o.autoreset, env.o.horizon)
        for k in STATE_KEYS:
            self.model.rows[k][c] = kids[k]
        return Expansion(rep['reward'], rep['done'], rep['result'], rep['info'])

    def expand_all(self, parents, first_child, from_envs=False, source=None, device=False):
        from gym_novel_gridworlds_amd.snapshot import all_actions_pairs
        p, a, c, shape = all_actions_pairs(parents, first_child, len(self.env.spec.actions_id))
        return self.expand(p, a, c, from_envs=from_envs, source=source, device=device).reshape(*shape)


class OracleVecExpand(SO.OracleVecSnap):
    """snapshot_oracle.OracleVecSnap whose snapshots expand: lets the host logic run without a GPU."""

    def snapshot(self, capacity=None):
        s = _BoundExpandSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s


sharded_on_oracle = functools.partial(T.sharded_on_oracle, OracleVecExpand)


def good_seed(spec, n, lo=4):
    return next(sd for sd in range(lo, lo + 40) if not Oracle(spec.compile(), n, seed=sd).reset() & 2)   # (tight maps can exhaust the placement)


__all__ = ['T', 'oracle_expand', 'rows_state', 'assert_rows', 'assert_reports', 'OracleVecExpand', 'sharded_on_oracle', 'good_seed', 'STATE_KEYS']
