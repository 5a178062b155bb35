"""Expected one-step lookahead tables from the unmodified CPU oracle: for every action, step a copy of the state with that action for all
envs and read reward, done, result, cost code, message code and message argument; the info words are assembled from those.  Nothing
here comes from the HIP path (tests/test_lookahead*.py compare the device's tables with these)."""
import numpy as np

import ngw_testlib as T
from mask_oracle import state_from  # noqa: F401  (re-exported: the tests build oracle states with it)
from oracle.ngw_oracle import Oracle


def oracle_lookahead(spec, st, autoreset=False, horizon=0):
    """{'reward' int32 [n, A], 'done' bool [n, A], 'result' bool [n, A], 'info' uint32 [n, A]}: column a = the oracle's outputs of
    step(a) from each env's state in `st` (a copy is stepped: `st` is untouched).  With autoreset the stepped copy resets where an episode
    ends; the outputs read are the terminal step's, as ngw_get_step_out reports them (done = 1 for goal and horizon, info bit 1 for the
    goal only)."""
    cs = spec.compile()
    A, n = cs.n_actions, st.n
    reward, done = np.zeros((n, A), np.int32), np.zeros((n, A), bool)
    result, info = np.zeros((n, A), bool), np.zeros((n, A), np.uint32)
    for a in range(A):
        o = Oracle(cs, n, autoreset=autoreset, horizon=horizon)
        o.st = st.copy()
        o.step(np.full(n, a, np.int32))
        reward[:, a], done[:, a], result[:, a], info[:, a] = o.reward, o.done.astype(bool), o.result.astype(bool), T.info_word(o)
    return dict(reward=reward, done=done, result=result, info=info)


def assert_table(got, exp, where):
    """Every entry of a lookahead table equals the oracle's; names the first env / action that differs."""
    for k in ('reward', 'done', 'result', 'info'):
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, "%s: %s shape %r expected %r" % (where, k, g.shape, e.shape)
        bad = np.argwhere(g != e)
        assert len(bad) == 0, "%s: %s differs in %d entries, first env %d action %d: got %r expected %r (info got %#x expected %#x)" % (
            where, k, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], e[tuple(bad[0])],
            int(np.asarray(got['info'])[tuple(bad[0])]), int(np.asarray(exp['info'])[tuple(bad[0])]))


class OracleVecLook(T.OracleVec):
    """T.OracleVec with VecNovelGridworld's lookahead(): lets the single-env adapter's and the wrappers' host logic run without a GPU."""

    def lookahead(self, device=False, copy=False):
        from gym_novel_gridworlds_amd.vec_env import Lookahead
        t = oracle_lookahead(self.spec, self.o.st, self.o.autoreset, self.o.horizon)
        return Lookahead(t['reward'], t['done'], t['result'], t['info'])

    def rebuild(self, spec):
        T.OracleVec.rebuild(self, spec)
        return self
