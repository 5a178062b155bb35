"""Expected plan evaluations from the unmodified CPU oracle: per plan, a fresh Oracle on a copy of the state is stepped T times; an env
stops accumulating at the first step whose `done` is set (goal, FireWall death, the horizon under autoreset) - that step counts.  The info
words are assembled from the oracle's outputs as tests/lookahead_oracle.py does.  Nothing here comes from the HIP path
(tests/test_plans*.py compare the device's results with these)."""
import numpy as np

import mask_oracle as M
import ngw_testlib as T
from oracle.ngw_oracle import Oracle


def oracle_plans(spec, st, plans, autoreset=False, horizon=0):
    """plans: integer [n, P, T], env-major, every id inside the action list.  {'ret' int32 [n, P], 'length' int32 [n, P], 'ended' bool
    [n, P], 'info' uint32 [n, P]}.  `st` is untouched (a copy is stepped; with autoreset the copy resets where an episode ends, which
    the masked accumulation never sees)."""
    cs = spec.compile()
    plans = np.asarray(plans)
    n, P, steps = plans.shape
    assert n == st.n
    ret, length = np.zeros((n, P), np.int32), np.zeros((n, P), np.int32)
    ended, info = np.zeros((n, P), bool), np.zeros((n, P), np.uint32)
    for p in range(P):
        o = Oracle(cs, n, autoreset=autoreset, horizon=horizon)
        o.st = st.copy()
        alive = np.ones(n, bool)
        for t in range(steps):
            o.step(np.ascontiguousarray(plans[:, p, t], np.int32))
            word = T.info_word(o)
            done = o.done.astype(bool)
            ret[alive, p] += o.reward[alive]
            length[alive, p] += 1
            info[alive, p] = word[alive]
            ended[:, p] |= alive & done
            alive &= ~done
            if not alive.any():
                break
    return dict(ret=ret, length=length, ended=ended, info=info)


def assert_plans(got, exp, where):
    """Every result equals the oracle's; names the first env / plan that differs."""
    for k in ('ret', 'length', 'ended', 'info'):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, "%s: %s shape %r expected %r" % (where, k, g.shape, e.shape)
        bad = np.argwhere(g != e)
        assert len(bad) == 0, "%s: %s differs in %d entries, first env %d plan %d: got %r expected %r (info got %#x expected %#x)" % (
            where, k, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], e[tuple(bad[0])],
            int(np.asarray(got['info'])[tuple(bad[0])]), int(np.asarray(exp['info'])[tuple(bad[0])]))


def solved_plans(cfg):
    """The recorded solved episodes of a fixture configuration as one plan per env: (spec, start state, plans [nso, 1, T] padded with Left
    to the longest, expected ret, expected length).  The recordings run a few steps PAST the goal (the reference's sticky done: every
    later step reports done with the forced reward); a plan stops at the first step that ends the episode, so what is expected is the
    recorded rewards' sum and the step count up to and including the first recorded done - and the recorded tail must be all done."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    cs = spec.compile()
    nso = T.spec_json()['cfgs'][cfg]['n_solved']
    K = len(spec.items_id)
    inv = np.stack([g['so%d_inv0' % k] if 'so%d_inv0' % k in g else np.zeros(K, np.int32) for k in range(nso)])
    st = M.state_from(spec, np.stack([g['so%d_map0' % k] for k in range(nso)]), np.stack([g['so%d_loc0' % k] for k in range(nso)]),
                      np.array([g['so%d_facing0' % k] for k in range(nso)]), inv, np.zeros(nso, np.int32))
    lens = [len(g['so%d_action' % k]) for k in range(nso)]
    plans = np.ones((nso, 1, max(lens)), np.int32)                   # Left = 1
    ret, length = [], []
    for k in range(nso):
        plans[k, 0, :lens[k]] = g['so%d_action' % k]
        done, reward = g['so%d_done' % k], g['so%d_reward' % k]
        first = int(np.argmax(done != 0))
        assert done[first] and done[first:].all() and (reward[first:] == cs.reward_done).all(), (cfg, k)
        ret.append(int(reward[:first + 1].sum()))
        length.append(first + 1)
    return spec, st, plans, ret, length


def PlanRows(e):
    """A single-env adapter's [P] results as the [1, P] arrays assert_plans compares."""
    return {k: np.asarray(e[k])[None] for k in ('ret', 'length', 'ended', 'info')}


class OracleVecPlans(T.OracleVec):
    """T.OracleVec with VecNovelGridworld's evaluate_plans() (host plans [N, P, T], validated the same way): lets the single-env adapter's,
    the wrappers' and the sharded env's host logic run without a GPU."""
    launches = 0

    def evaluate_plans(self, plans, device=False, copy=False):
        from gym_novel_gridworlds_amd.vec_env import PlanEval
        a = np.asarray(plans)
        assert a.dtype.kind in 'iu' and a.ndim == 3 and a.shape[0] == self.num_envs
        bad = (a < 0) | (a >= len(self.spec.actions_id))
        if bad.any():
            raise ValueError("%d is not in list" % int(a[bad][0]))
        self.launches += 1
        t = oracle_plans(self.spec, self.o.st, a, self.o.autoreset, self.o.horizon)
        return PlanEval(t['ret'], t['length'], t['ended'], t['info'])

    def rebuild(self, spec):
        T.OracleVec.rebuild(self, spec)
        return self
