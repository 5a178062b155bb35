"""Expected valid-action random playouts from the unmodified CPU oracle.  Per step of the pairs still alive: the mask words of their current
rows (mask_oracle.oracle_mask_words: every action stepped on a copy), the Philox word from the oracle library's own generator
(ngwo_philox4x32_10) under the counter and key of include/ngw.h, the k-th set bit - a chooser - and one step of pairs_oracle.step_pairs, in two
copies: one under the handle's autoreset setting and horizon for the reports, one that never resets for the end rows.  Nothing
here imports gym_novel_gridworlds_amd.playout or touches the HIP path (tests/test_playout*.py compare both with these)."""
import numpy as np

import expand_oracle as XO
import mask_oracle as M
import pairs_oracle as PA
import slot_rollout_oracle as RO
from oracle.ngw_oracle import lib

STATE_KEYS = RO.STATE_KEYS
PLAYOUT_TAG = 0x504C4159
REPORTS = ('ret', 'length', 'ended', 'info', 'first_action')


def philox_word(seed, pair, t):
    """Word t & 3 of the block the contract names for global pair number `pair` at step t."""
    seed, pair, t = int(seed), int(pair), int(t)
    ctr = np.array([t >> 2, 0, pair & 0xFFFFFFFF, pair >> 32], np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) ^ PLAYOUT_TAG], np.uint32)
    out = np.zeros(4, np.uint32)
    lib().ngwo_philox4x32_10(ctr, key, out)
    return int(out[t & 3])


def choose(mask_word, seed, pair, t, n_actions):
    """The contract's choice for one pair, in Python integers."""
    m = int(mask_word)
    if m == 0:
        m = (1 << n_actions) - 1
    k = (philox_word(seed, pair, t) * bin(m).count('1')) >> 32
    for a in range(64):
        if (m >> a) & 1:
            if k == 0:
                return a
            k -= 1
    raise AssertionError("k beyond the set bits")


def drawn(spec, seed, first_pair, pick):
    """A chooser for pairs_oracle.step_pairs: the mask word of every pair's current row (0 where no action would succeed) and
    pick(word, pair number, t) -> the action."""
    def chooser(t, idx, now):
        words = M.oracle_mask_words(spec, XO.rows_state(spec, now, np.arange(len(idx))))
        return np.array([pick(w, first_pair + int(j), t) for w, j in zip(words, idx)], np.int32), dict(masks=words)
    return chooser


def played(e):
    """step_pairs' record as the playout oracles return it."""
    return e['ends'], dict(e['reports'], first_action=e['actions'][0].copy()), e['actions'], PA.kept(e, 'masks', np.uint64)


def oracle_playout(spec, rows, parents, steps, seed, first_pair=0, autoreset=False, horizon=0):
    """-> (ends, reports, actions, masks): ends = {key: [count, ...]} the seven arrays of the rows as the last executed step leaves them,
    reports = {'ret' int32, 'length' int32, 'ended' bool, 'info' uint32, 'first_action' int32}, each [count], actions int32 [steps, count]
    (-1: not executed), masks uint64 [steps, count]: the mask word before each executed step (0 elsewhere - and where no action would
    succeed).  `rows` is untouched."""
    A = spec.compile().n_actions
    return played(PA.step_pairs(spec, rows, parents, steps, drawn(spec, seed, first_pair, lambda w, pair, t: choose(w, seed, pair, t, A)), None,
                                autoreset, horizon))


def assert_playout(got, exp, exp_actions, where):
    """The five reports of `got` (a Playout of numpy arrays) and - where recorded - its actions equal the oracle's."""
    RO.assert_reports(got, exp, where)
    g = np.asarray(got['first_action'])
    bad = np.nonzero(g != exp['first_action'])[0]
    assert bad.size == 0, "%s: first_action differs in %d pairs, first pair %d: got %d expected %d" % (where, bad.size, bad[0], g[bad[0]], exp['first_action'][bad[0]])
    if got['actions'] is not None:
        a = np.asarray(got['actions'])
        assert a.shape == exp_actions.shape and a.dtype == np.int32, (where, a.shape, a.dtype)
        bad = np.argwhere(a != exp_actions)
        assert not len(bad), "%s: actions differ at %d places, first (step, pair) %s: got %d expected %d" % (
            where, len(bad), tuple(bad[0]), a[tuple(bad[0])], exp_actions[tuple(bad[0])])


class _BoundPlayoutSnapshot(RO._BoundRolloutSnapshot):
    """slot_rollout_oracle's bound snapshot with Snapshot.playout: the product's host checks (snapshot.check_playout), the oracle's steps."""

    def playout(self, parents, steps, seed, children=None, from_envs=False, source=None, first_pair=0, record=False, device=False):
        from gym_novel_gridworlds_amd.snapshot import check_playout
        rows, n_parents, own = self._source('playout', from_envs, source)
        env = self.env
        p, c, count, steps = check_playout(parents, steps, children, n_parents, self.capacity, own)
        p = np.arange(count) if p is None else p
        ends, rep, acts, _ = oracle_playout(env.spec, rows, p, steps, seed, first_pair, env.o.autoreset, env.o.horizon)
        if c is not None:
            for k in STATE_KEYS:
                self.model.rows[k][c] = ends[k]
        return rep, (acts if record else None)


class OracleVecPlayout(RO.OracleVecRollout):
    """slot_rollout_oracle.OracleVecRollout whose snapshots play out: lets the host logic run without a GPU."""

    def snapshot(self, capacity=None):
        s = _BoundPlayoutSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s


__all__ = ['oracle_playout', 'assert_playout', 'choose', 'philox_word', 'OracleVecPlayout', 'STATE_KEYS', 'REPORTS']
