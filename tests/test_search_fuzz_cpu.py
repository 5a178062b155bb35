"""The search fuzz's own evidence, without a GPU: the walk of tests/test_search_fuzz.py - same seeds, same chunks - on an oracle-backed stand-in
(search_fuzz_standin.StandIn) passes, which pins the driver and proves every draw executable; over all chunks it executes every call kind and
every form of the pair calls, and few calls are refused; and five seeded faults in the stand-in each make run_case raise.

Coverage of the committed seed (NGW_FUZZ_SEED = 7100, six chunks, 67 cases; executed / refused per kind, then the pair calls per form and source) is
asserted below as conditions and printed by `pytest -s`; the whole walk takes about 9 s on the CPU, 0.9 - 2.0 s per chunk.  Every kind is executed
9 - 33 times, every (pair call, form, source) cell 1 - 7 times, 2 of 606 calls are refused (successor keys beyond 34 x 34 maps) and no case ends in
"Cannot place items"."""
import collections

import numpy as np
import pytest

import search_fuzz as F
import search_fuzz_standin as SI
import snapshot_oracle as SO
import slot_rollout_oracle as RO
from test_search_fuzz import CHUNKS, SEED

PAIR_KINDS = {'srollout': F.ROLLOUT_FORMS, 'srollout_kids': F.ROLLOUT_FORMS, 'splayout': F.PLAYOUT_FORMS, 'splayout_kids': F.PLAYOUT_FORMS}
_walk = {}


def walk():
    """The stand-in walk of every chunk, once per session: -> Counter of (kind, 'executed' / 'refused' / ..., form)."""
    if not _walk:
        cov = collections.Counter()
        for chunk in range(CHUNKS):
            rs = np.random.RandomState(SEED + chunk)
            for case, cfg in enumerate(F.chunk_cfgs(chunk, CHUNKS)):
                F.run_case(rs, cfg, case, SI.make_stand_in, lambda kind, status, form: cov.update([(kind, status, form)]))
        _walk['cov'] = cov
    return _walk['cov']


def test_the_same_walk_passes_on_the_stand_in():
    cov = walk()
    cases = sum(v for (k, _, _), v in cov.items() if k == '(case)')
    assert cases == len(F.T.CFGS)


def test_coverage_of_the_committed_seed():
    cov = walk()
    executed, refused = collections.Counter(), collections.Counter()
    for (kind, status, form), v in cov.items():
        if kind != '(case)':
            (executed if status == 'executed' else refused)[kind] += v
    for kind in sorted(F.KINDS):
        print('%-18s executed %3d refused %2d' % (kind, executed[kind], refused[kind]))
    for kind, forms in sorted(PAIR_KINDS.items()):
        for form in forms:
            print('%-18s %-9s from slots %2d from envs %2d' % (kind, form, cov[(kind, 'executed', form + '/slots')], cov[(kind, 'executed', form + '/envs')]))
    for form in F.PLAYOUTS_FORMS:
        print('%-18s %-9s %2d' % ('playouts', form, cov[('playouts', 'executed', form)]))
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
    assert n_ref <= 0.15 * (n_exec + n_ref), (n_exec, n_ref)
    cases = sum(v for (k, _, _), v in cov.items() if k == '(case)')
    placement = sum(v for (k, s, _), v in cov.items() if k == '(case)' and s == 'placement')
    assert placement <= 0.10 * cases, (placement, cases)


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


@pytest.mark.parametrize('faulty', [CommitsPlayout, StaleMasks, RestoreTakesEpisode, ExpandReadsSlots, AlwaysFresh], ids=lambda c: c.__name__)
def test_seeded_faults_are_caught(faulty):
    """Each defect, within at most one chunk of the committed walk."""
    rs = np.random.RandomState(SEED)
    with pytest.raises(AssertionError):
        for case, cfg in enumerate(F.chunk_cfgs(0, CHUNKS)):
            F.run_case(rs, cfg, case, lambda **kw: faulty(**kw))
