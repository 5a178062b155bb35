"""Expected weighted choices among valid actions from the unmodified CPU oracle.  The mask words are mask_oracle's (every action stepped on a
copy), the Philox word is the oracle library's own generator (ngwo_philox4x32_10) under the counter and key of include/ngw.h, and the
selection is written out here pair by pair in Python scalars: np.float32 adds in action order, one multiply, the first cumulative sum above
the threshold.  A weighted playout is playout_oracle's chooser with this choice in the place of the uniform one.  Nothing here imports
gym_novel_gridworlds_amd.sample or touches the HIP path (tests/test_sample*.py compare both with these)."""
import functools

import numpy as np

import expand_oracle as XO
import mask_oracle as M
import ngw_testlib as T
import pairs_oracle as PA
import playout_oracle as PO
from oracle.ngw_oracle import lib

STATE_KEYS = PO.STATE_KEYS
SAMPLE_TAG = 0x53414D50
F_BAD_WEIGHT = 16
LO, HI = np.float32(2.0 ** -64), np.float32(2.0 ** 64)


def philox_word(tag, seed, pair, t):
    """Word t & 3 of the block the contract names for global pair number `pair` at step number t under `tag`."""
    seed, pair, t = int(seed), int(pair), int(t)
    ctr = np.array([t >> 2, 0, pair & 0xFFFFFFFF, pair >> 32], np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) ^ tag], np.uint32)
    out = np.zeros(4, np.uint32)
    lib().ngwo_philox4x32_10(ctr, key, out)
    return int(out[t & 3])


def is_bad(x):
    """Does this weight raise F_BAD_WEIGHT?"""
    x = np.float32(x)
    return bool(np.isnan(x) or x < 0 or x > HI)


def select(mask_word, x, w, n_actions):
    """Rules 1 and 3 - 6 for one pair, in Python integers and np.float32 scalars: -> (action, mass, m)."""
    m = int(mask_word)
    if m == 0:
        m = (1 << n_actions) - 1
    x = np.asarray(x, np.float32)
    assert x.shape == (n_actions,)
    v, c, acc = [], [], np.float32(0)
    for a in range(n_actions):
        xa = x[a]
        ok = (m >> a) & 1 and not np.isnan(xa) and LO <= xa <= HI
        v.append(xa if ok else np.float32(0))
        acc = np.float32(acc + v[-1])
        c.append(acc)
    mass = acc
    if mass > 0:
        u = np.float32(np.float32(w >> 8) * np.float32(2.0 ** -24))
        assert float(u) == (w >> 8) / 16777216.0
        thr = np.float32(u * mass)
        for a in range(n_actions):
            if v[a] > 0 and c[a] > thr:
                return a, mass, m
        return max(a for a in range(n_actions) if v[a] > 0), mass, m
    k = (w * bin(m).count('1')) >> 32
    for a in range(64):
        if (m >> a) & 1:
            if k == 0:
                return a, np.float32(0), m
            k -= 1
    raise AssertionError("k beyond the set bits")


def choose(mask_words, weights, seed, pairs, t, n_actions, tag=SAMPLE_TAG):
    """The contract for every pair: weights [count, A] -> (action int32, mass float32, m uint64), each [count]."""
    out = [select(mw, x, philox_word(tag, seed, p, t), n_actions) for mw, x, p in zip(mask_words, weights, pairs)]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.uint64))


def oracle_sample(spec, rows, idx, weights, seed, first_pair=0, t=0):
    """-> (action, mass, m, flag): the expected Sampled fields for rows idx of `rows` under weights [count, A]; flag = F_BAD_WEIGHT or 0."""
    A = spec.compile().n_actions
    idx = np.asarray(idx, np.int64)
    words = M.oracle_mask_words(spec, XO.rows_state(spec, rows, idx))
    weights = np.asarray(weights, np.float32)
    action, mass, m = choose(words, weights, seed, [first_pair + j for j in range(len(idx))], t, A)
    return action, mass, m, F_BAD_WEIGHT if any(is_bad(x) for x in weights.reshape(-1)) else 0


def oracle_weighted_playout(spec, rows, parents, steps, seed, weights, first_pair=0, autoreset=False, horizon=0):
    """playout_oracle.oracle_playout with the weighted choice (weights [A]) on the playout's own mask word and Philox word (PLAYOUT_TAG):
    -> (ends, reports, actions, masks) as there."""
    A = spec.compile().n_actions
    weights = np.asarray(weights, np.float32)
    pick = lambda w, pair, t: select(w, weights, PO.philox_word(seed, pair, t), A)[0]                    # noqa: E731
    return PO.played(PA.step_pairs(spec, rows, parents, steps, PO.drawn(spec, seed, first_pair, pick), None, autoreset, horizon))


def assert_sampled(got, exp, where):
    """action, mass bits and mask word of `got` (a Sampled of numpy arrays) equal exp = (action, mass, m, ...): exact, no tolerance."""
    ga, gm, gw = np.asarray(got[0]), np.asarray(got[1]), np.asarray(got[2])
    assert ga.dtype == np.int32 and gm.dtype == np.float32 and gw.dtype == np.uint64, (where, ga.dtype, gm.dtype, gw.dtype)
    assert ga.shape == exp[0].shape == gm.shape == gw.shape, (where, ga.shape, exp[0].shape)
    bad = np.nonzero((ga != exp[0]) | (gm.view(np.uint32) != exp[1].view(np.uint32)) | (gw != exp[2]))[0]
    assert bad.size == 0, "%s: %d pairs differ, first pair %d: got (%d, %r, %#x) expected (%d, %r, %#x)" % (
        where, bad.size, bad[0], ga[bad[0]], gm[bad[0]], int(gw[bad[0]]), exp[0][bad[0]], exp[1][bad[0]], int(exp[2][bad[0]]))


def random_weights(rs, count, n_actions, bad=False):
    """float32 [count, A] spanning 2^-70 .. 2^64 - and, with `bad`, on to 2^70 with a negative, a NaN, an infinity and 2^65 written in -; a
    fifth of them zero."""
    x = np.exp2(rs.uniform(-70, 70 if bad else 64, (count, n_actions))).astype(np.float32)
    x[rs.rand(count, n_actions) < 0.2] = 0
    if bad:
        for val in (-1.0, np.nan, np.inf, 2.0 ** 65):
            x[rs.randint(count), rs.randint(n_actions)] = val
    return x


class OracleVecSample(PO.OracleVecPlayout):
    """playout_oracle.OracleVecPlayout with VecNovelGridworld's sample_actions / playouts on the host: lets the adapter's, the wrappers' and the
    sharded env's forwarding run without a GPU."""

    def __init__(self, spec, num_envs=1, seed=0, env_index_base=0, **kw):
        super().__init__(spec, num_envs, seed=seed, env_index_base=env_index_base, **kw)
        self.env_index_base, self.flags = env_index_base, 0

    @property
    def n_actions(self):
        return len(self.spec.actions_id)

    def sample_actions(self, weights, seed, t=0, envs=None, device=False):
        from gym_novel_gridworlds_amd.sample import Sampled
        idx = np.arange(self.num_envs) if envs is None else np.asarray(envs)
        w = np.asarray(weights)
        if w.shape != (len(idx), self.n_actions):
            raise ValueError("weights: an array of shape %s expected" % [len(idx), self.n_actions])
        a, mass, m, flag = oracle_sample(self.spec, self.o.st, idx, w, seed, self.env_index_base, t)
        self.flags |= flag
        return Sampled(a, mass, m)

    def playouts(self, n_playouts, steps, seed, device=False, weights=None):
        return self._playouts(n_playouts, steps, seed, weights)

    def _playouts(self, n_playouts, steps, seed, weights, more=None):
        """The one body of every stand-in's playouts(): the uniform or the weighted playout of P pairs per env; more(parents, actions) -> the
        fields a richer result holds after Playout's six, and its class."""
        from gym_novel_gridworlds_amd.playout import Playout
        P, N = int(n_playouts), self.num_envs
        parents = np.repeat(np.arange(N), P)
        tail = (self.env_index_base * P, self.o.autoreset, self.o.horizon)
        if weights is None:
            _, rep, acts, _ = PO.oracle_playout(self.spec, self.o.st, parents, steps, seed, *tail)
        else:
            _, rep, acts, _ = oracle_weighted_playout(self.spec, self.o.st, parents, steps, seed, weights, *tail)
        play = Playout(rep['ret'], rep['length'], rep['ended'], rep['info'], rep['first_action'], None)
        if more is not None:
            cls, fields = more(parents, acts)
            play = cls(*play, *fields)
        return play.shaped(N, P)


sharded_on_oracle = functools.partial(T.sharded_on_oracle, OracleVecSample)
