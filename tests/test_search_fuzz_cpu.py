"""The search fuzz's own evidence, without a GPU: the walk of tests/test_search_fuzz.py - same seeds, same chunks - on an oracle-backed stand-in
(search_fuzz_standin.StandIn) passes, which pins the driver and proves every draw executable; over all chunks it executes every call kind and
every form of the pair calls, and few calls are refused; and nine seeded faults in the stand-in each make run_case raise.

Coverage of the committed seed (NGW_FUZZ_SEED = 7100, six chunks, 67 cases; executed / refused per kind, then the pair calls per form and source) is
asserted below as conditions and printed by `pytest -s`; the whole walk takes about 16 s on the CPU, 2.2 - 3.7 s per chunk (9 s before the guided
kinds and the 'view' forms, which replay every playout once more for the views and twice more for the offer and the guided simulation).  Every kind
is executed 4 - 40 times, every (pair call, form, source) cell 1 - 7 times, 2 of 618 calls are refused (successor keys beyond 34 x 34 maps) and no
case ends in "Cannot place items".  The pair kinds and playouts weigh 6 - 7 in search_fuzz.KINDS so that every cell of the wider table stays covered.

The 49 guided pair calls and 5 guided playouts() of the walk (test_coverage_of_the_guided_calls, from guided_playout_oracle's event counts on the
model side): both `outside` rules from slots and from envs, limits together with 'stop', both observations, calls without default weights, calls
that offer nothing and find the table as earlier calls left it, maps of 24 x 24 and more; hits and misses each above 20 % of the executed steps,
re-entries, zero-mass rows, steps whose action differs from the default's, steps that look up key 0 - reachable under KEY_INV alone (an empty
inventory), never under KEY_INV | KEY_SELECTED, whose second term is never absent -, and tables in which two members share a home bucket."""
import collections
import time

import numpy as np
import pytest

import guided_playout_oracle as GO
import search_fuzz as F
import search_fuzz_standin as SI
import snapshot_oracle as SO
import slot_rollout_oracle as RO
from test_search_fuzz import CHUNKS, PROBED_CHUNKS, SEED

PAIR_KINDS = {'srollout': F.ROLLOUT_FORMS, 'srollout_kids': F.ROLLOUT_FORMS, 'splayout': F.PLAYOUT_FORMS, 'splayout_kids': F.PLAYOUT_FORMS}
EVENTS = ('hits', 'misses', 'executed', 'reentries', 'zero_mass', 'differs', 'key0', 'displaced', 'shared_home')
_walk = {}


def walk():
    """The stand-in walk of every chunk, once per session: -> (Counter of (kind, 'executed' / 'refused' / ..., form), the guided calls' records - one
    dict each, with its chunk -, the largest key count a table reached, the seconds per chunk)."""
    if not _walk:
        cov, guided, sizes, seconds = collections.Counter(), [], [0], []
        for chunk in range(CHUNKS):
            def log(kind, status, form):
                if kind == '(guided)':
                    guided.append(dict(form, kind=status, chunk=chunk))
                elif kind == '(table)':
                    sizes.append(form)
                else:
                    cov.update([(kind, status, form)])
            t0 = time.time()
            rs = np.random.RandomState(SEED + chunk)
            for case, cfg in enumerate(F.chunk_cfgs(chunk, CHUNKS)):
                F.run_case(rs, cfg, case, SI.make_stand_in, log)
            seconds.append(time.time() - t0)
        _walk.update(cov=cov, guided=guided, largest=max(sizes), seconds=seconds)
    return _walk['cov'], _walk['guided'], _walk['largest'], _walk['seconds']


def test_the_same_walk_passes_on_the_stand_in():
    cov, _, largest, _ = walk()
    cases = sum(v for (k, _, _), v in cov.items() if k == '(case)')
    assert cases == len(F.T.CFGS)
    assert largest <= F.TABLE_CAPACITY, largest


def test_coverage_of_the_committed_seed():
    cov, _, largest, seconds = walk()
    executed, refused = collections.Counter(), collections.Counter()
    for (kind, status, form), v in cov.items():
        if kind != '(case)':
            (executed if status == 'executed' else refused)[kind] += v
    for kind in sorted(F.KINDS):
        print('%-20s executed %3d refused %2d' % (kind, executed[kind], refused[kind]))
    for kind, forms in sorted(PAIR_KINDS.items()):
        for form in forms:
            print('%-20s %-9s from slots %2d from envs %2d' % (kind, form, cov[(kind, 'executed', form + '/slots')], cov[(kind, 'executed', form + '/envs')]))
    for kind in F.GUIDED_KINDS:
        print('%-20s %-9s from slots %2d from envs %2d' % (kind, 'guided', cov[(kind, 'executed', 'guided/slots')], cov[(kind, 'executed', 'guided/envs')]))
    for form in F.PLAYOUTS_FORMS:
        print('%-20s %-9s %2d' % ('playouts', form, cov[('playouts', 'executed', form)]))
    print('largest table %d keys; seconds per chunk %s' % (largest, ' '.join('%.1f' % s for s in seconds)))
    for kind in F.KINDS:
        assert executed[kind] >= 3, "%s was executed %d times" % (kind, executed[kind])
    for kind, forms in PAIR_KINDS.items():
        for form in forms:
            for source in ('slots', 'envs'):
                assert cov[(kind, 'executed', '%s/%s' % (form, source))] >= 1, (kind, form, source)
    for form in F.PLAYOUTS_FORMS:
        assert cov[('playouts', 'executed', form)] >= 1, form
    for kind, form in (('restore', 'keep'), ('restore', 'episode'), ('copy', 'within'), ('copy', 'between'), ('expand', 'slots'), ('expand', 'envs'),
                       ('expand_all', 'slots'), ('expand_all', 'envs')):
        assert cov[(kind, 'executed', form)] >= 1, (kind, form)
    n_exec, n_ref = sum(executed.values()), sum(refused.values())
    print('%d calls, %d refused' % (n_exec + n_ref, n_ref))
    assert n_ref <= 0.15 * (n_exec + n_ref), (n_exec, n_ref)
    cases = sum(v for (k, _, _), v in cov.items() if k == '(case)')
    placement = sum(v for (k, s, _), v in cov.items() if k == '(case)' and s == 'placement')
    assert placement <= 0.10 * cases, (placement, cases)


def test_coverage_of_the_guided_calls():
    """What the guided playouts of the committed walk met, from the model side alone (guided_playout_oracle's event counts, carried by the logger)."""
    cov, guided, _, _ = walk()
    pairs = [g for g in guided if g['kind'] in F.GUIDED_KINDS]
    for kind in F.GUIDED_KINDS:
        assert executed_guided(guided, kind) >= 6, kind
        assert executed_guided(guided, kind) == cov[(kind, 'executed', 'guided/slots')] + cov[(kind, 'executed', 'guided/envs')]
    for outside in ('stop', 'default'):
        for source in ('slots', 'envs'):
            assert any(g['outside'] == outside and g['source'] == source for g in pairs), (outside, source)
    assert any(g['limits'] and g['outside'] == 'stop' for g in pairs), "limits together with outside='stop'"
    for observe in ('lidar', 'agent_view'):
        assert any(g['observe'] == observe for g in pairs), observe
    assert any(not g['default'] for g in pairs), "a call without default weights"
    assert any(not g['offered'] for g in pairs), "a call that offered no keys: a table only earlier calls filled"
    assert any(not g['offered'] and g['members'] and g['hits'] for g in guided), "... and found states of its own in it"
    assert any(g['S'] >= 24 for g in pairs), "a configuration whose 64 staged maps exceed 64 KiB"
    assert not any(g['bound'] for g in guided), "no offer of the committed walk is held back by the table's capacity"
    tot = {k: sum(g[k] for g in guided) for k in EVENTS}
    print('guided calls %d (playouts form %d): %s' % (len(guided), len(guided) - len(pairs), tot))
    assert tot['hits'] >= 0.2 * tot['executed'] and tot['misses'] >= 0.2 * tot['executed'], tot
    assert tot['reentries'] >= 1 and tot['zero_mass'] >= 1 and tot['differs'] >= 1, tot
    assert tot['key0'] >= 1, "no executed step looked up key 0 (reachable under KEY_INV alone, with an empty inventory)"
    assert tot['displaced'] >= 1, "every member key sits in its home bucket"
    # the GPU side asserts a member outside its home bucket for the chunks named there: two members that share a home bucket cannot both sit in it
    shared = tuple(c for c in range(CHUNKS) if any(g['shared_home'] for g in guided if g['chunk'] == c))
    print('chunks with two members in one home bucket:', shared)
    assert shared == PROBED_CHUNKS, shared


def executed_guided(guided, kind):
    return sum(1 for g in guided if g['kind'] == kind)


# ---------------------------------------------------------------- seeded faults: a fuzz that cannot fail proves nothing
class CommitsPlayout(SI.StandIn):
    """(a) playouts() commits its first step to env 0."""

    def playouts(self, n_playouts, steps, seed, **kw):
        r = super().playouts(n_playouts, steps, seed, **kw)
        rows = SO.oracle_state(self.o)
        RO._step_rows(self.spec, self.spec.compile(), rows, np.array([0]), np.array([int(np.asarray(r.first_action).reshape(-1)[0])]), False, 0)
        SO.put_state(self.o, rows)
        return r


class StaleMasks(SI.StandIn):
    """(b) restore leaves the action-mask words of the restored envs as they were."""
    _stale = None

    def snapshot(self, capacity=None):
        env, s = self, super().snapshot(capacity)
        plain = s.restore

        def restore(slots=None, envs=None, keep_episode=False):
            words = SI.M.oracle_mask_words(env.spec, env.o.st)
            e = np.arange(env.num_envs) if envs is None else np.asarray(SI.un(envs))
            plain(slots, envs, keep_episode)
            env._stale = (e, words[e])
        s.restore = restore
        return s

    def action_mask_words(self, device=False, copy=False):
        w = super().action_mask_words()
        if self._stale is not None:
            w[self._stale[0]] = self._stale[1]
        return w

    def _step(self, a):
        self._stale = None
        super()._step(a)


class RestoreTakesEpisode(SI.StandIn):
    """(c) restore(keep_episode=True) overwrites the episode counter."""

    def snapshot(self, capacity=None):
        s = super().snapshot(capacity)
        plain = s.restore
        s.restore = lambda slots=None, envs=None, keep_episode=False: plain(slots, envs, False)
        return s


class ExpandReadsSlots(SI.StandIn):
    """(d) expand with from_envs=True reads slot rows instead of the live envs."""

    def snapshot(self, capacity=None):
        s = super().snapshot(capacity)
        plain = s.expand

        def expand(parents, actions, children, from_envs=False, source=None, device=False):
            if from_envs and not np.isin(SI.un(children), SI.un(parents)).any():
                return plain(parents, actions, children, from_envs=False, source=None)
            return plain(parents, actions, children, from_envs=from_envs, source=source)
        s.expand = expand
        return s


class AlwaysFresh(SI.StandIn):
    """(e) KeyTable.insert reports `fresh` for a key already present."""

    def key_table(self, capacity):
        t = super().key_table(capacity)
        plain = t.insert

        def insert(keys, device=False):
            found = plain(keys)
            return SI.KeyInsert(found.where, found.fresh | (found.where >= 0))
        t.insert = insert
        return t


class LooksUpTheKeyItLeaves(SI.StandIn):
    """(f) a guided playout looks up the key of the state step t LEAVES, not the one it is in: `where` and `depth` are one state late."""

    @staticmethod
    def _guided(spec, rows, parents, steps, seed, members, row_fn, *rest):
        e = GO.oracle_guided(spec, rows, parents, steps, seed, members, row_fn, *rest)
        held, ran = set(int(k) for k in members), e['actions'] >= 0
        e['before'] = np.where(ran, e['keys'], 0).astype(np.uint64)
        e['hit'] = ran & np.array([[int(k) in held for k in row] for row in e['before'].tolist()], bool).reshape(ran.shape)
        e['depth'] = np.cumprod(e['hit'], 0).sum(0).astype(np.int32)
        return e


class StopRunsTheStep(SI.StandIn):
    """(g) outside='stop' executes the step it should have stopped at (under the default weights), and stops after it."""

    @staticmethod
    def _guided(spec, rows, parents, steps, seed, members, row_fn, default, first_pair, autoreset, horizon, fields, limits, stop, lc):
        e = GO.oracle_guided(spec, rows, parents, steps, seed, members, row_fn, default, first_pair, autoreset, horizon, fields, limits, stop, lc)
        if not stop:
            return e
        length = e['reports']['length'].astype(np.int64)
        lim = np.full(len(length), steps, np.int64) if limits is None else np.clip(np.asarray(limits, np.int64), 0, steps)
        cut = ~e['reports']['ended'] & (length < lim)                          # the pairs the table stopped
        return GO.oracle_guided(spec, rows, parents, steps, seed, members, row_fn, default, first_pair, autoreset, horizon, fields, length + cut, False, lc)


class DepthCountsEveryHit(SI.StandIn):
    """(h) `depth` counts every executed in-table step, not only the leading ones."""

    @staticmethod
    def _guided(*args):
        e = GO.oracle_guided(*args)
        e['depth'] = (e['hit'] & (e['actions'] >= 0)).sum(0).astype(np.int32)
        return e


class ViewsRepeatBlockZero(SI.StandIn):
    """(i) observe='agent_view' re-emits block 0's window in every later block of the steps a pair executed."""

    def _views(self, obs, length):
        obs = {k: v.copy() for k, v in obs.items()}
        for t in range(1, obs['agent_map'].shape[0]):
            ran = np.asarray(length) >= t
            obs['agent_map'][t, ran] = obs['agent_map'][0, ran]
        return obs


# (the fault, the chunk of the committed walk that catches it: the first with a call that meets it)
FAULTS = [(CommitsPlayout, 0), (StaleMasks, 0), (RestoreTakesEpisode, 2), (ExpandReadsSlots, 2), (AlwaysFresh, 0), (LooksUpTheKeyItLeaves, 0),
          (StopRunsTheStep, 0), (DepthCountsEveryHit, 0), (ViewsRepeatBlockZero, 0)]


@pytest.mark.parametrize('faulty, chunk', [pytest.param(f, c, id=f.__name__) for f, c in FAULTS])
def test_seeded_faults_are_caught(faulty, chunk):
    """Each defect, within at most one chunk of the committed walk."""
    rs = np.random.RandomState(SEED + chunk)
    with pytest.raises(AssertionError):
        for case, cfg in enumerate(F.chunk_cfgs(chunk, CHUNKS)):
            F.run_case(rs, cfg, case, lambda **kw: faulty(**kw))
