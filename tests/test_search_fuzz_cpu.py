"""The search fuzz's own evidence, without a GPU: the walk of tests/test_search_fuzz.py - same seeds, same chunks - on an oracle-backed stand-in
(search_fuzz_standin.StandIn) passes, which pins the driver and proves every draw executable; over all chunks it executes every call kind and
every form of the pair calls, and few calls are refused; and eighteen seeded faults in the stand-in each make run_case raise.

Coverage of the committed seed (NGW_FUZZ_SEED = 7632, six chunks, 67 cases of 8 - 15 calls; executed / refused per kind, then the pair calls per
form and source) is asserted below as conditions and printed by `pytest -s`; the whole walk takes about 19 s on the CPU, 2.4 - 4.0 s per chunk.
Every kind is executed 5 - 41 times, 2 of 756 calls are refused (successor keys beyond 34 x 34 maps), the largest table holds 649 keys and no
case ends in "Cannot place items".  The pair kinds, playouts and the six newest kinds weigh 6 - 7 in search_fuzz.KINDS so that every cell of the
wider table stays covered.

The 37 guided pair calls, 38 frontier_twins calls and 3 guided playouts() of the walk (test_coverage_of_the_guided_calls, from
guided_playout_oracle's event counts on the model side): both `outside` rules from slots and from envs, limits together with 'stop', both
observations, calls without default weights, calls that offer nothing and find the table as earlier calls left it, maps of 24 x 24 and more; hits
and misses each above 20 % of the executed steps, re-entries, zero-mass rows, steps whose action differs from the default's, steps that look up key
0 - reachable under KEY_INV alone (an empty inventory), never under KEY_INV | KEY_SELECTED, whose second term is never absent -, and tables in
which two members share a home bucket.

test_coverage_of_the_new_kinds_and_the_padded_lists holds the walk to: every new kind (slot_walk, walk, walk_go, frontier_compact, frontier_step,
frontier_twins) in every chunk, every call with a device list padded at least once, a list with every pair skipped met by each kernel that returns
before its stage-in (expand, slot rollout, playout, successors, slot lidar), a short frontier limit, a compaction across a tile border from a
non-zero byte offset, a walk_go with an unreachable item.  Seeded faults j - r: the skipped pair, the compaction, the allocation, the walk."""
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
NOTES = ('(pad)', '(walk)', '(walk_go)', '(compact)', '(step)', '(twins)')
_notes, _per_chunk = [], collections.Counter()
NEW_KINDS = ('slot_walk', 'walk', 'walk_go', 'frontier_compact', 'frontier_step', 'frontier_twins')
# the calls that take a device index list, and the kernels that return before their stage-in when a ballot finds no live pair, by the kinds that launch them
LIST_KINDS = ('save', 'restore', 'fork', 'copy', 'expand', 'srollout', 'srollout_kids', 'splayout', 'splayout_kids', 'splayout_guided',
              'splayout_guided_kids', 'slot_lidar', 'slot_view', 'slot_masks', 'slot_keys', 'slot_insert_keys', 'state_keys', 'succ_keys',
              'insert_state_keys', 'insert_succ_keys', 'sample') + NEW_KINDS[:3] + NEW_KINDS[4:]        # (frontier_compact takes no index list)
EARLY_RETURN = {'expand': ('expand', 'frontier_step'), 'slot rollout': ('srollout', 'srollout_kids', 'walk_go'),
                'playout': ('splayout', 'splayout_kids', 'frontier_twins') + F.GUIDED_KINDS, 'successors': ('succ_keys', 'insert_succ_keys', 'frontier_step'),
                'slot lidar': ('slot_lidar',)}


def coverage_gaps(notes, per_chunk):
    """The conditions on the new kinds and the padded lists that a walk does NOT meet (the committed seed: none)."""
    gaps = []
    for kind in NEW_KINDS:
        gaps += ['%s not executed in chunk %d' % (kind, c) for c in range(CHUNKS) if per_chunk[(c, kind)] < 1]
    padded = collections.Counter(k for note, _, k, _ in notes if note == '(pad)')
    gaps += ['%s never padded' % k for k in LIST_KINDS if padded[k] < 1]
    for kernel, kinds in sorted(EARLY_RETURN.items()):
        if not any(note == '(pad)' and k in kinds and form[0] == 'all' for note, _, k, form in notes):
            gaps.append('%s never met a list with every pair skipped' % kernel)
    if not any(note == '(step)' and form[1] for note, _, _, form in notes):
        gaps.append('frontier_step never met a short limit')
    if not any(note == '(compact)' and form[0] > F.FRONTIER_TILE and form[1] != 0 for note, _, _, form in notes):
        gaps.append('frontier_compact never crossed a tile border at a non-zero byte offset')
    if not any(note == '(walk_go)' and form[0] > 0 for note, _, _, form in notes):
        gaps.append('walk_go never met an unreachable item')
    return gaps


def test_coverage_of_the_new_kinds_and_the_padded_lists():
    walk()
    print(collections.Counter((note, k) + (form[:2] if note == '(pad)' else ()) for note, _, k, form in _notes))
    assert coverage_gaps(_notes, _per_chunk) == []


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
                elif kind in NOTES:                       # what the padded calls, the walks and the frontiers met: (note, chunk, kind, details)
                    _notes.append((kind, chunk, status, form))
                else:
                    cov.update([(kind, status, form)])
                    if status == 'executed':
                        _per_chunk.update([(chunk, kind)])
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


class NoneRaisesBadIndex(SI.StandIn):
    """(j) a pair whose index is IDX_NONE raises F_BAD_INDEX."""

    def _skip(self, gone):
        self._flags |= SI.F_BAD_INDEX


class NoneChildGoesToSlotZero(SI.StandIn):
    """(k) the child of a pair whose destination is IDX_NONE is written into slot 0."""

    def _live(self, parents, children, gone):
        return parents != SI.NONE, np.where(children == SI.NONE, 0, children)


class StaleRowsWhenAllSkipped(SI.StandIn):
    """(l) a list with every pair skipped returns the rows of the row staged last instead of the skip values: the stale stage-in."""

    @staticmethod
    def _blank(out, gone, fill=0):
        return out if gone.all() else SI.blank_rows(out, gone, fill)


class CompactionLosesTheSecondTile(SI.StandIn):
    """(m) the compaction ranks the hits of the second tile of 4096 flags from 0 again."""

    @staticmethod
    def _compact(flags, div, map, capacity):
        first, second, count, full = SI.FO.compact(flags, div, map, capacity)
        raw = np.ascontiguousarray(flags).reshape(-1).view(np.uint8)
        hits = F.FRONTIER_TILE + np.flatnonzero(raw[F.FRONTIER_TILE:2 * F.FRONTIER_TILE])[:len(first)]      # (their entries land on the first tile's)
        first, second = first.copy(), second.copy()
        first[:len(hits)] = hits // div if map is None else np.asarray(map)[hits // div]
        second[:len(hits)] = hits % div
        return first, second, count, full


class AllocLeavesTheCursor(SI.StandIn):
    """(n) alloc hands out slots and leaves the cursor where it was."""

    @staticmethod
    def _alloc(count, cursor, limit, capacity):
        slots, _, full = SI.FO.alloc(count, cursor, limit, capacity)
        return slots, cursor, full


class AllocIgnoresTheLimit(SI.StandIn):
    """(o) alloc hands out slots beyond the limit."""

    @staticmethod
    def _alloc(count, cursor, limit, capacity):
        return SI.FO.alloc(count, cursor, 1 << 30, capacity)


class ForwardEntersAnything(SI.StandIn):
    """(p) the walk lets Forward enter a cell that does not hold id 0."""

    def _walk_moves(self, cells, S, p):
        r, c, f = p
        fr, fc = r + SI.DR[f], c + SI.DC[f]
        return ([(fr, fc, f)] if 0 <= fr < S and 0 <= fc < S else []) + [(r, c, SI.LEFT[f]), (r, c, SI.RIGHT[f])]


class GoalTiesByColumnFirst(SI.StandIn):
    """(q) the walk breaks goal ties by (D, c, r, f)."""

    def _goal_rank(self, d, r, c, f):
        return (d, c, r, f)


class LengthClampedToSteps(SI.StandIn):
    """(r) walk_plans' `length` is clamped to `steps`."""

    def _walk_length(self, length, steps):
        return min(length, steps)


# (the fault, the chunk of the committed walk that catches it: the first with a call that meets it)
FAULTS = [(CommitsPlayout, 0), (StaleMasks, 0), (RestoreTakesEpisode, 3), (ExpandReadsSlots, 1), (AlwaysFresh, 0), (LooksUpTheKeyItLeaves, 0),
          (StopRunsTheStep, 0), (DepthCountsEveryHit, 0), (ViewsRepeatBlockZero, 0), (NoneRaisesBadIndex, 0), (NoneChildGoesToSlotZero, 0),
          (StaleRowsWhenAllSkipped, 0), (CompactionLosesTheSecondTile, 1), (AllocLeavesTheCursor, 0), (AllocIgnoresTheLimit, 0),
          (ForwardEntersAnything, 0), (GoalTiesByColumnFirst, 0), (LengthClampedToSteps, 0)]


@pytest.mark.parametrize('faulty, chunk', [pytest.param(f, c, id=f.__name__) for f, c in FAULTS])
def test_seeded_faults_are_caught(faulty, chunk):
    """Each defect, within at most one chunk of the committed walk."""
    rs = np.random.RandomState(SEED + chunk)
    with pytest.raises(AssertionError):
        for case, cfg in enumerate(F.chunk_cfgs(chunk, CHUNKS)):
            F.run_case(rs, cfg, case, lambda **kw: faulty(**kw))
