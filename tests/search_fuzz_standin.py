"""An oracle-backed stand-in with the whole search surface of VecNovelGridworld, for the CPU walk of tests/search_fuzz.py: the existing
stand-ins composed by inheritance (trajectory_oracle.OracleVecTraj and its bases, successor_key_oracle.OracleVecSuccessors,
lookahead_oracle.OracleVecLook, plan_oracle.OracleVecPlans, key_table_oracle.stand_in_table for the table's host checks) and the surface they lack
written from the row-level reference functions.  Settings it has no notion of are accepted and ignored (prepared episodes, the page-locked block,
the fused lidar's format); a "device" input is the host array in the device form's layout, wrapped in Dev.  A guided playout reads its weight rows
from the caller's table_weights at the buckets of the stand-in's OWN table (guided_result), so the driver's rows and buckets are checked too.
An index list may hold IDX_NONE: that pair is skipped - its outputs are what include/ngw.h stores for it, nothing is written, no flag -; walk_distances
/ walk_plans are a layered search of their own from the contract text, frontier() a Frontier over frontier_oracle with host arrays.  No GPU."""
import numpy as np

import frontier_oracle as FO
import guided_playout_oracle as GO
import key_table_oracle as KT
import lookahead_oracle as LO
import mask_oracle as M
import plan_oracle as PL
import playout_oracle as PO
import sample_oracle as SA
import search_fuzz as F
import slot_observe_oracle as OO
import snapshot_oracle as SO
import state_key_oracle as SK
import successor_key_oracle as SU
import trajectory_oracle as TO
import trajectory_view_oracle as VO
from gym_novel_gridworlds_amd.key_table import KeyInsert, check_keys
from gym_novel_gridworlds_amd.playout import Playout, PlayoutGuided, PlayoutPath, PlayoutTraj
from gym_novel_gridworlds_amd.sample import Sampled
from gym_novel_gridworlds_amd.snapshot import Expansion, MapsTooLarge, SuccessorKeys, insert_successors
from gym_novel_gridworlds_amd.state_keys import unique_of_keys
from gym_novel_gridworlds_amd.vec_env import PLACEMENT_MESSAGE, PlanEval, RolloutPath, RolloutTraj
from gym_novel_gridworlds_amd.walk import WalkPlans, plan_action_ids
from oracle import ngw_oracle as NO

STATE_KEYS = SO.STATE_KEYS
F_BAD_WEIGHT = 16                    # include/ngw.h NGW_F_BAD_WEIGHT: a weight row that was read holds a negative, infinite or NaN entry
F_BAD_INDEX = 4                      # NGW_F_BAD_INDEX
NONE = FO.IDX_NONE                   # NGW_IDX_NONE: a pair that is not there - skipped, and no flag
PAIR_FILL = dict(first_action=-1, actions=-1, where=-1)        # what a rollout / playout stores for a skipped pair: -1 in these, 0 in every other field
PER_PAIR = ('ret', 'length', 'ended', 'info', 'first_action', 'depth')
DR, DC = (-1, 1, 0, 0), (0, 0, -1, 1)                         # facing NORTH 0, SOUTH 1, WEST 2, EAST 3
LEFT, RIGHT = (2, 3, 1, 0), (3, 2, 0, 1)


class Dev:
    """A host array that stands for a device tensor: the layout is the device form's."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)

    def __getitem__(self, key):
        return Dev(self.a[key])


def un(x):
    return x.a if isinstance(x, Dev) else x


def gone_of(*lists):
    """bool [count]: the pairs of which ANY index is IDX_NONE, or None where every pair is there."""
    gone = None
    for x in lists:
        x = un(x)
        if x is not None and np.ndim(x) == 1:
            m = np.asarray(x) == NONE
            gone = m if gone is None else gone | m
    return gone if gone is not None and gone.any() else None


def blank_result(got, gone):
    """A rollout / playout result with a skipped pair's values in the places of the pairs in `gone`."""
    new = {}
    for f in got._fields:
        x = getattr(got, f)
        if x is None:
            continue
        fill = PAIR_FILL.get(f, 0)
        if isinstance(x, dict):
            new[f] = {k: blank_axis(v, gone, 1, fill) for k, v in x.items()}
        else:
            new[f] = blank_axis(x, gone, 0 if f in PER_PAIR else 1, fill)
    return got._replace(**new)


def blank_axis(x, gone, axis, fill):
    x = np.array(x)
    x[(slice(None),) * axis + (gone,)] = fill
    return x


def is_dev(x):
    return isinstance(x, Dev)


def pair_result(kind, e, record, path_keys, traj):
    rep = e['rep']
    if kind == 'rollout':
        head = [rep['ret'], rep['length'], rep['ended'], rep['info']]
        if traj:
            return RolloutTraj(*head, e['keys'], e['rewards'], e['obs'])
        return RolloutPath(*head, e['keys']) if path_keys else PlanEval(*head)
    head = [rep['ret'], rep['length'], rep['ended'], rep['info'], rep['first_action'], e['actions'] if record else None]
    if traj:
        return PlayoutTraj(*head, e['keys'], e['rewards'], e['masks'], e['obs'])
    return PlayoutPath(*head, e['keys']) if path_keys else Playout(*head)


def run_pairs(env, kind, rows, parents, record=False, observe=None, view_size=5, table=None, table_weights=None, outside='default', **kw):
    """One rollout / playout call of any form on the dict `rows` -> (the result as the product types it, the end rows)."""
    lc = env.lidar if observe == 'lidar' else None
    views = int(view_size) if observe == 'agent_view' else None
    traj = observe is not None or kw.get('rewards') or kw.get('masks')
    kw['limits'] = un(kw.get('limits'))
    kw['weights'] = un(kw.get('weights'))
    if kind == 'rollout':
        kw.pop('weights')
    if kw.get('fields') is None:
        kw['fields'] = SK.STATE
    if table is not None:
        return guided_result(env, rows, parents, record, lc, views, table, un(table_weights), outside, **kw)
    e = F.ref_pairs(env.spec, rows, parents, kind, env.o.autoreset, env.o.horizon, lc=lc, view_size=views, **kw)
    if views is not None:
        e['obs'] = env._views(e['obs'], e['rep']['length'])
    return pair_result(kind, e, record, kw.get('path_keys'), traj), e['ends']


def guided_result(env, rows, parents, record, lc, views, table, tw, outside, steps, seed, first_pair=0, weights=None, limits=None, path_keys=False,
                  fields=SK.STATE, rewards=False, masks=False):
    """A guided playout from guided_playout_oracle's forward simulation.  The members are the keys this stand-in's own table holds, and the weight row
    of a member is read from the caller's table_weights at the bucket that table gave the key - never the driver's row function: rows written into
    the wrong buckets, or another tensor, change the actions or (a NaN row) raise the weight flag here as on the device."""
    assert isinstance(table, StandInTable) and table.env is env, "table: a key table of this env expected"
    A = len(env.spec.actions_id)
    tw = np.asarray(tw)
    assert tw.dtype == np.float32 and tw.shape == (table.buckets, A), ("table_weights", tw.dtype, tw.shape)
    order = table.model.order
    e = env._guided(env.spec, rows, parents, steps, seed, list(order), lambda k: tw[order[int(k)]], weights, first_pair, env.o.autoreset, env.o.horizon,
                    fields, limits, outside == 'stop', lc)
    if e['bad']:
        env._flags |= F_BAD_WEIGHT
    where = np.full(e['hit'].shape, -1, np.int32)
    for t, j in np.argwhere(e['hit']):
        where[t, j] = order[int(e['before'][t, j])]
    obs = e['obs']
    if views is not None:
        obs = env._views(VO.expect_views(env.spec, rows, parents, e, views), e['reports']['length'])
    rep = e['reports']
    got = PlayoutGuided(rep['ret'], rep['length'], rep['ended'], rep['info'], e['actions'][0].copy(), e['actions'] if record else None,
                        e['keys'] if path_keys else None, e['rewards'] if rewards else None, e['masks'] if masks else None, obs, where,
                        np.asarray(e['depth'], np.int32))
    return got, e['ends']


class StandInSnapshot(PO._BoundPlayoutSnapshot, SU._BoundSuccessorSnapshot):
    """The bound snapshots of the existing stand-ins, with every form of rollout / playout, copy, the slot observers, keys and the key-table calls."""

    def _there(self, a, b):
        """The copies of a save / restore / copy that are there: a skipped one is a no-op."""
        a, b = un(a), un(b)
        gone = gone_of(a, b)
        if gone is None:
            return a, b
        self.env._skip(gone)
        return np.asarray(a)[~gone], np.asarray(b)[~gone]

    def save(self, envs=None, slots=None):
        super().save(*self._there(envs, slots))

    def restore(self, slots=None, envs=None, keep_episode=False):
        super().restore(*self._there(slots, envs), keep_episode)

    def copy(self, src_slots, dst_slots, source=None):
        src = self if source is None else source
        s, d = self._there(src_slots, dst_slots)
        for k in STATE_KEYS:
            self.model.rows[k][d] = src.model.rows[k][s]

    def _parent_rows(self, from_envs, source):
        return self.env.o.st if from_envs else (self if source is None else source).model

    def expand(self, parents, actions, children, from_envs=False, source=None, device=False):
        p, a, c = un(parents), un(actions), un(children)
        gone = gone_of(p, c)
        if gone is None:
            return super().expand(p, a, c, from_envs=from_envs, source=source)
        self.env._skip(gone)
        live, c = self.env._live(np.asarray(p), np.asarray(c), gone)
        rep = [np.zeros(len(p), t) for t in (np.int32, bool, bool, np.uint32)]           # a skipped pair's reports: the zeros they were allocated as
        if live.any():
            for x, y in zip(rep, super().expand(np.asarray(p)[live], np.asarray(a)[live], c[live], from_envs=from_envs, source=source)):
                x[live] = y
        return Expansion(*rep)

    def expand_all(self, parents, first_child, from_envs=False, source=None, device=False):
        return super().expand_all(un(parents), first_child, from_envs=from_envs, source=source)

    def _pairs(self, kind, parents, children, from_envs, source, record=False, **kw):
        env, p, c = self.env, np.asarray(un(parents)), un(children)
        rows, gone = F.rows_of(self._parent_rows(from_envs, source)), gone_of(p, c)
        if gone is not None:
            # the pairs of one call do not see each other and a playout draws by the pair's position: a pair that is not there runs from a spare row
            # (env 0's state, a legal one) behind the source's rows, and what it returned is blanked
            env._skip(gone)
            rows = {k: np.concatenate([rows[k], getattr(env.o.st, k)[:1]]) for k in STATE_KEYS}
            p = np.where(p == NONE, len(rows['facing']) - 1, p)
        got, ends = run_pairs(env, kind, rows, p, record, **kw)
        if c is not None:
            live, c = (slice(None), c) if gone is None else env._live(np.asarray(un(parents)), np.asarray(c), gone)
            for k in STATE_KEYS:
                self.model.rows[k][c[live]] = ends[k][live]
        return got if gone is None else blank_result(got, gone)

    def _by_row(self, idx, fn, fill=0):
        return by_row(self.env, idx, fn, fill)

    def rollout(self, parents, plans, children=None, from_envs=False, source=None, device=False, limits=None, path_keys=False, fields=SK.STATE, rewards=False,
                masks=False, observe=None, view_size=5):
        plans = np.asarray(un(plans)).T if is_dev(plans) or device else np.asarray(plans)     # (device plans are step-major: walk_plans' own layout)
        return self._pairs('rollout', parents, children, from_envs, source, plans=plans, limits=limits, path_keys=path_keys, fields=fields, rewards=rewards,
                           observe=observe, view_size=view_size)

    def playout(self, parents, steps, seed, children=None, from_envs=False, source=None, first_pair=0, record=False, device=False, weights=None, limits=None,
                path_keys=False, fields=SK.STATE, rewards=False, masks=False, observe=None, view_size=5, table=None, table_weights=None, outside='default'):
        return self._pairs('playout', parents, children, from_envs, source, record=record, steps=steps, seed=seed, first_pair=first_pair, weights=weights,
                           limits=limits, path_keys=path_keys, fields=fields, rewards=rewards, masks=masks, observe=observe, view_size=view_size, table=table,
                           table_weights=table_weights, outside=outside)

    def lidar_observation(self, slots=None, device=False):
        return self._by_row(slots, lambda i: OO.expect_lidar(self.env.spec, self.env.lidar, self.model.rows, i))

    def agent_view(self, slots=None, view_size=5, device=False):
        return self._by_row(slots, lambda i: OO.expect_view(self.model.rows, i, view_size))

    def action_masks(self, slots=None, device=False):
        return self._by_row(slots, lambda i: OO.expect_masks(self.env.spec, self.model.rows, i))

    def keys(self, slots=None, fields=SK.STATE, device=False):
        return self._by_row(slots, lambda i: F.fast_keys(F.rows_at(self.model, i), fields))

    def walk_distances(self, slots=None, device=False):
        return walk_result(self.env, self.model.rows, np.arange(self.capacity) if slots is None else slots, None, 0)

    def walk_plans(self, slots, items, steps, device=False):
        return walk_result(self.env, self.model.rows, np.arange(self.capacity) if slots is None else slots, items, steps)

    def frontier(self, capacity):
        return StandInFrontier(self, capacity)

    def unique(self, slots=None, fields=SK.STATE, device=False):
        return unique_of_keys(self.keys(slots, fields))

    def insert_keys(self, table, slots=None, fields=SK.STATE, device=False):
        keys = self.keys(slots, fields)
        return keys, table.insert(keys)

    def successor_keys(self, slots=None, fields=SK.STATE, device=False, reports=True):
        self.env._succ_limit()
        return successors_there(self.env, un(slots), lambda s: super(StandInSnapshot, self).successor_keys(s, fields, reports=reports), reports)

    def insert_successor_keys(self, table, slots=None, fields=SK.STATE, device=False):
        s = self.successor_keys(slots, fields)
        found = table.insert(s.keys.reshape(-1))
        return s, KeyInsert(found.where.reshape(s.keys.shape), found.fresh.reshape(s.keys.shape))


def by_row(env, idx, fn, fill=0):
    """fn(rows) - an array, or a dict of arrays, of one row per index - with `fill` in the rows of the indices that are not there: "its output row is
    all zeros", "that key is 0".  (The rows that are not there are computed for a row that is - the list's first, or row 0 - and overwritten.)"""
    idx = np.asarray(un(idx))
    gone = gone_of(idx)
    if gone is None:
        return fn(idx)
    env._skip(gone)
    return env._blank(fn(np.where(gone, idx[~gone][0] if (~gone).any() else 0, idx)), gone, fill)


def blank_rows(out, gone, fill=0):
    if isinstance(out, dict):
        return {k: blank_axis(v, gone, 0, fill) for k, v in out.items()}
    return blank_axis(out, gone, 0, fill)


def successors_there(env, s, call, reports):
    """SuccessorKeys of a list with parents that are not there: their A keys and reports are 0."""
    gone = gone_of(s)
    if gone is None:
        return call(s)
    env._skip(gone)
    s, A = np.asarray(s), len(env.spec.actions_id)
    if gone.all():
        got = SuccessorKeys(np.zeros((len(s), A), np.uint64), *([np.zeros((len(s), A), t) for t in (np.int32, bool, bool, np.uint32)] if reports else [None] * 4))
    else:
        got = call(np.where(gone, s[~gone][0], s))
    return SuccessorKeys(*[None if x is None else blank_axis(x, gone, 0, 0) for x in got])


# ---- walk distances and go-to plans, from the contract text of include/ngw.h (ngw_snapshot_walk): a layered search over (r, c, f)
def walk_search(env, cells, S, pose, K):
    """-> ({pose: D}, [the goal pose of item k or None])."""
    D, layer = {pose: 0}, [pose]
    while layer:
        after = []
        for p in layer:
            for q in env._walk_moves(cells, S, p):
                if q not in D:
                    D[q] = D[p] + 1
                    after.append(q)
        layer = after
    best = [None] * K
    for (r, c, f), d in D.items():
        fr, fc = r + DR[f], c + DC[f]
        if 0 <= fr < S and 0 <= fc < S and 0 <= cells[fr * S + fc] < K:
            k, rank = cells[fr * S + fc], env._goal_rank(d, r, c, f)
            if best[k] is None or rank < best[k][0]:
                best[k] = (rank, (r, c, f))
    return D, [None if b is None else b[1] for b in best]


def walk_back(cells, S, D, goal, ids):
    """The moves to `goal`: walking back, the Forward predecessor first, then the pose that reaches it by Left, then the one that reaches it by Right."""
    q, moves = goal, []
    for d in range(D[goal], 0, -1):
        r, c, f = q
        pr, pc = r - DR[f], c - DC[f]
        if 0 <= pr < S and 0 <= pc < S and cells[r * S + c] == 0 and D.get((pr, pc, f)) == d - 1:
            moves.append(ids[0]); q = (pr, pc, f)
        elif D.get((r, c, RIGHT[f])) == d - 1:
            moves.append(ids[1]); q = (r, c, RIGHT[f])
        else:
            moves.append(ids[2]); q = (r, c, LEFT[f])
    return moves[::-1]


def walk_result(env, rows, idx, items, steps):
    """walk_distances (items None) / walk_plans of rows idx: -1 in every output of a row whose index or item is not there."""
    K, S = len(env.spec.items_id), env.spec.map_size
    idx, items = np.asarray(un(idx)), un(items)
    count = len(idx)
    if items is not None:
        ids = plan_action_ids(env.spec.compile())
        items = np.full(count, items) if np.ndim(items) == 0 else np.asarray(items)
    gone = gone_of(idx, items)
    if gone is not None:
        env._skip(gone)
    dist = np.full((count, K), -1, np.int32)
    plans, length = np.full((max(steps, 0), count), -1, np.int32), np.full(count, -1, np.int32)
    seen = {}
    for j in range(count):
        if gone is not None and gone[j]:
            continue
        i = int(idx[j])
        if i not in seen:
            cells = [int(x) for x in np.asarray(rows['map'][i]).reshape(-1)]
            seen[i] = (cells,) + walk_search(env, cells, S, (int(rows['loc'][i][0]), int(rows['loc'][i][1]), int(rows['facing'][i])), K)
        cells, D, goals = seen[i]
        dist[j] = [-1 if g is None else D[g] for g in goals]
        if items is not None and goals[int(items[j])] is not None:
            moves = walk_back(cells, S, D, goals[int(items[j])], ids)
            plans[:min(len(moves), steps), j] = moves[:steps]
            length[j] = env._walk_length(len(moves), steps)
    return dist if items is None else WalkPlans(plans, length, dist)


class StandInFrontier:
    """frontier.Frontier over frontier_oracle: the lists, the two counts and the cursor are host arrays."""

    def __init__(self, snap, capacity):
        self.snap, self.env, self.capacity = snap, snap.env, int(capacity)
        self.first, self.second, self.slots = [np.full(self.capacity, NONE, np.int32) for _ in range(3)]
        self.count_dev, self.cursor = np.zeros(2, np.int32), np.zeros(1, np.int32)

    def compact(self, flags, div=1, map=None):
        self.first, self.second, count, full = self.env._compact(np.asarray(un(flags)), int(div), None if map is None else np.asarray(un(map)), self.capacity)
        self.count_dev = np.array(count, np.int32)
        self.env._flags |= FO.F_FRONTIER_FULL if full else 0
        return self.first, self.second

    def alloc(self, limit=None):
        limit = self.snap.capacity if limit is None else limit
        self.slots, cursor, full = self.env._alloc(int(self.count_dev[0]), int(self.cursor[0]), limit, self.capacity)
        self.cursor = np.array([cursor], np.int32)
        self.env._flags |= FO.F_FRONTIER_FULL if full else 0
        return self.slots

    def reset_cursor(self, start=0):
        self.cursor = np.array([start], np.int32)

    def count(self):
        return int(self.count_dev[0])

    def total(self):
        return int(self.count_dev[1])

    def fresh_pairs(self, fresh, parents=None):
        return self.compact(fresh, int(np.shape(un(fresh))[1]), parents)

    def fresh_steps(self, fresh):
        return self.compact(fresh, max(int(np.shape(un(fresh))[1]), 1))

    def transitions(self, result):
        """(step t, pair j) of every step the result's pairs executed: t < length[j]; the steps are the first per-step field's."""
        length = np.asarray(result.length).reshape(1, -1)
        steps = [int(np.shape(x)[0]) for x in (getattr(result, f, None) for f in ('rewards', 'masks', 'keys', 'actions')) if x is not None][0]
        return self.compact(np.arange(steps)[:, None] < length, max(length.shape[1], 1))

    def tree_steps(self, result):
        """(bucket, action, t, j) of every executed in-table step (where >= 0) of a guided playout recorded with its actions."""
        steps = int(np.shape(result.where)[0])
        w, a = np.asarray(result.where).reshape(steps, -1), np.asarray(result.actions).reshape(steps, -1)
        t, j = self.compact(w >= 0, max(w.shape[1], 1))
        live = t != NONE
        pick = lambda x: np.where(live, x[t * live, j * live], NONE).astype(np.int32)       # noqa: E731
        return pick(w), pick(a), t, j

    def close(self):
        self.first = self.second = self.slots = None


class StandInTable:
    """KeyTable over key_table_oracle's model; the host-side argument checks are the product's (a stand_in_table runs them)."""

    def __init__(self, env, capacity):
        self.env, self.checks = env, KT.stand_in_table(capacity, env)
        self.buckets, self.capacity, self.model = self.checks.buckets, capacity, KT.KeyTableModel()

    def _keys(self, keys):
        k, _ = check_keys(un(keys))
        return k.view(np.uint64)

    def insert(self, keys, device=False):
        k = self._keys(keys)
        fresh, stored = self.model.insert(k)
        where = np.array([self.model.order[int(x)] if s else -1 for x, s in zip(k.tolist(), stored)], np.int32).reshape(len(k))
        return KeyInsert(where, fresh)

    def lookup(self, keys, device=False):
        return np.array([self.model.order.get(int(x), -1) for x in self._keys(keys).tolist()], np.int32)

    def __len__(self):
        return len(self.model)


class StandIn(TO.OracleVecTraj, SU.OracleVecSuccessors, LO.OracleVecLook, PL.OracleVecPlans):
    device = 0

    def __init__(self, spec, num_envs=1, seed=0, autoreset=False, horizon=0, env_index_base=0, terminal_capture=False, **ignored):
        super().__init__(spec, num_envs, seed=seed, env_index_base=env_index_base, autoreset=autoreset, horizon=horizon)
        self.term_on, self._flags, self._graph = bool(terminal_capture), 0, None
        n, S, K = num_envs, spec.map_size, len(spec.items_id)
        self._term = dict(map=np.zeros((n, S, S), np.int8), agent_location=np.zeros((n, 2), np.int32), agent_facing_id=np.zeros(n, np.int32),
                          inventory_items_quantity=np.zeros((n, K), np.int32))

    _h = True

    def to_device(self, a):
        return Dev(a)

    def ptr_of(self, x):
        return x

    # ---- the handle's own calls
    def _step(self, a):
        o = self.o
        a = np.ascontiguousarray(a, np.int32)
        if self.term_on and o.autoreset:
            o2 = NO.Oracle(o.cspec, o.n, autoreset=False)
            o2.st = o.st.copy()
            o2.step(a)
        self._flags |= int(o.step(a))
        if self.term_on and o.autoreset:
            idx = np.nonzero(o.done)[0]
            t = self._term
            t['map'].reshape(o.n, -1)[idx] = o2.st.map[idx]
            t['agent_location'][idx], t['agent_facing_id'][idx], t['inventory_items_quantity'][idx] = o2.st.loc[idx], o2.st.facing[idx], o2.st.inv[idx]

    def _raise_flags(self):
        if self._flags & 2:
            raise AssertionError(PLACEMENT_MESSAGE)

    def error_flags(self):
        f = self._flags                                  # ngw_error_flags "reads and clears" (the placement flag stays for _raise_flags)
        self._flags &= 2
        return f

    def step(self, actions, copy=False, with_obs=True):
        self._step(actions)
        o, st = self.o, self.o.st
        self._raise_flags()
        info = {'result': o.result.astype(bool), 'step_cost_code': o.cost_code, 'message_code': o.msg_code, 'message_arg': o.msg_arg}
        obs = {'map': st.map, 'agent_location': st.loc, 'agent_facing_id': st.facing, 'inventory_items_quantity': st.inv}
        return obs, o.reward.copy(), o.done.astype(bool), info

    def step_device_many(self, acts, stride, k):
        for i in range(k):
            self._step(un(acts)[i])

    rollout_actions = step_device_many

    def rollout(self, n_steps, action_seed=1234, t0=0):
        self._flags |= int(self.o.rollout(n_steps, action_seed, t0))

    def graph_build(self, acts, stride, k):
        self._graph = un(acts)[:k].copy()

    def graph_launch(self, reps=1):
        for _ in range(reps):
            for a in self._graph:
                self._step(a)

    def terminal_observation(self, device=False):
        return self._term

    def set_action_masks(self, on=True):
        pass

    def lidar_configure(self, lidar_config=None, num_beams=8, fused=False, dtype=np.int32):
        super().lidar_configure(lidar_config, num_beams, fused, dtype)
        self._lidar_c = self.lidar.compile(self.spec)

    def lidar_observation(self, device=False, copy=False):
        st = self.o.st
        return NO.lidar(self._lidar_c, self.spec.map_size, len(self.spec.items_id), st.map, st.loc, st.facing, st.inv)

    def lidar_widen(self, pair, dtype=np.int32):
        return np.concatenate([pair[0].astype(dtype), pair[1].astype(dtype)], 1)

    def action_mask_words(self, device=False, copy=False):
        return M.oracle_mask_words(self.spec, self.o.st)

    def snapshot(self, capacity=None):
        s = StandInSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s

    def fork(self, src, keep_episode=False):
        src = un(src)
        gone = gone_of(src)
        if gone is None:
            return super().fork(src, keep_episode)
        s = self.snapshot()                              # an env whose source is not there keeps its state
        s.save()
        s.restore(slots=src, envs=np.where(gone, NONE, np.arange(self.num_envs)), keep_episode=keep_episode)
        s.close()

    def key_table(self, capacity):
        return StandInTable(self, capacity)

    def evaluate_plans(self, plans, device=False, copy=False):
        return super().evaluate_plans(un(plans).transpose(2, 1, 0) if is_dev(plans) else plans)

    def state_keys(self, envs=None, fields=SK.STATE, device=False):
        return by_row(self, np.arange(self.num_envs) if envs is None else envs, lambda i: F.fast_keys(F.rows_at(self.o.st, i), fields))

    def walk_distances(self, envs=None, device=False):
        return walk_result(self, F.rows_of(self.o.st), np.arange(self.num_envs) if envs is None else envs, None, 0)

    def walk_plans(self, items, steps, envs=None, device=False):
        return walk_result(self, F.rows_of(self.o.st), np.arange(self.num_envs) if envs is None else envs, items, steps)

    def insert_state_keys(self, table, envs=None, fields=SK.STATE, device=False):
        keys = self.state_keys(envs, fields)
        return keys, table.insert(keys)

    def _succ_limit(self):
        if self.spec.map_size > F.SUCC_MAX_MAP:
            raise MapsTooLarge("map_size %d: beyond the successor keys' two sets of rows" % self.spec.map_size)

    def successor_keys(self, envs=None, fields=SK.STATE, device=False, reports=True):
        self._succ_limit()
        return successors_there(self, un(envs), lambda e: super(StandIn, self).successor_keys(e, fields, reports=reports), reports)

    def insert_successor_keys(self, table, envs=None, fields=SK.STATE, device=False):
        s = self.successor_keys(envs, fields)
        found = table.insert(s.keys.reshape(-1))
        return s, KeyInsert(found.where.reshape(s.keys.shape), found.fresh.reshape(s.keys.shape))

    def sample_actions(self, weights, seed, t=0, envs=None, device=False):
        w, envs = un(weights).T if is_dev(weights) else weights, un(envs)
        gone = gone_of(envs)
        if gone is None:
            return super().sample_actions(w, seed, t, envs)
        self._skip(gone)                                 # (the draw goes by the pair's position: env 0 stands in, and the pair is blanked - action -1, mass 0, word 0)
        s = super().sample_actions(w, seed, t, np.where(gone, 0, envs))
        return Sampled(blank_axis(s.action, gone, 0, -1), blank_axis(s.mass, gone, 0, 0), blank_axis(s.mask_words, gone, 0, 0))

    def step_sampled(self, weights, seed, t=0):
        s = self.sample_actions(weights, seed, t)
        self._step(s.action)
        return s

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, observe=None, view_size=5, table=None, **kw):
        if observe != 'agent_view' and table is None:
            return super().playouts(n_playouts, steps, seed, weights=un(weights), observe=observe, **kw)
        P, N = int(n_playouts), self.num_envs
        got, _ = run_pairs(self, 'playout', F.rows_of(self.o.st), np.repeat(np.arange(N), P), steps=steps, seed=seed, first_pair=self.env_index_base * P,
                           weights=weights, observe=observe, view_size=view_size, table=table, **kw)
        return got.shaped(N, P)

    # ---- what the seeded faults of tests/test_search_fuzz_cpu.py replace
    _guided = staticmethod(GO.oracle_guided)
    _compact = staticmethod(FO.compact)
    _alloc = staticmethod(FO.alloc)
    _blank = staticmethod(blank_rows)

    def _views(self, obs, length):
        return obs

    def _skip(self, gone):
        """Pairs that are not there were met: no flag."""

    def _live(self, parents, children, gone):
        """-> (the pairs whose child is written, the slots): a pair with any index that is not there writes nothing."""
        return ~gone, children

    def _walk_moves(self, cells, S, p):
        """The poses one move from p: Forward iff the cell in front is inside the map and holds id 0, Left, Right."""
        r, c, f = p
        fr, fc = r + DR[f], c + DC[f]
        ahead = [(fr, fc, f)] if 0 <= fr < S and 0 <= fc < S and cells[fr * S + fc] == 0 else []
        return ahead + [(r, c, LEFT[f]), (r, c, RIGHT[f])]

    def _goal_rank(self, d, r, c, f):
        return (d, r, c, f)

    def _walk_length(self, length, steps):
        return length


def make_stand_in(**kw):
    return StandIn(**kw)
