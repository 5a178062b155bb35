"""The model of a search run (include/ngw.h ngw_search_start / ngw_search_run; gym_novel_gridworlds_amd/search.py): the seven steps of an
iteration with plain Python loops on the CPU oracle - the children and their info words from tests/expand_oracle.py, the table from
tests/key_value_oracle.py, the compaction and the slot allocation from tests/frontier_oracle.py, the selection of the k cheapest written
out here.  Written from the contract text and not from search.py (whose relax_reference tests/test_search_run_cpu.py holds to a statement
of its own).  Buckets have no model: the table's tags number the entries of `links`, as in key_value_oracle.label_correcting, and a goal is
(value, key).  Nothing here comes from the HIP path."""
import numpy as np

import expand_oracle as XO
import frontier_oracle as FO
import key_value_oracle as KV

NONE, IDX_NONE = KV.NONE, KV.IDX_NONE
I32_MIN = -(1 << 31)
STATE_KEYS = XO.STATE_KEYS


def step_cost_table(scale=1):
    from gym_novel_gridworlds_amd.spec import STEP_COSTS
    return [int(round(c * scale)) for c in STEP_COSTS]


def select(values, flags, keep, div, capacity):
    """The `keep` candidates (flag set, value not NONE) with the smallest (value, position), as entries (position // div, position % div) in
    ascending position order, IDX_NONE behind them -> (first, second, [taken, candidates])."""
    cand = sorted((int(values[p]), p) for p in range(len(values)) if flags[p] and int(values[p]) != NONE)
    chosen = sorted(p for _, p in cand[:keep])
    first, second = [IDX_NONE] * capacity, [IDX_NONE] * capacity
    for k, p in enumerate(chosen):
        first[k], second[k] = p // div, p % div
    return first, second, [len(chosen), len(cand)]


class SearchModel:
    """A search of `capacity` parents over a pool of `pool_capacity` rows.  costs: None - the step costs by the info word's cost code, times
    `scale`, rounded - or one cost per action."""

    def __init__(self, spec, capacity, pool_capacity, costs=None, scale=1, keep=None, stop_at_goals=False):
        self.spec, self.A = spec, spec.compile().n_actions
        self.capacity, self.pool_capacity, self.keep, self.stop = int(capacity), int(pool_capacity), keep, bool(stop_at_goals)
        self.costs = None if costs is None else [int(c) for c in costs]
        self.lut = step_cost_table(scale)
        self.table = KV.KeyValueModel()
        self.links = self.table.links = []
        self.rows = None                                # the pool: {name: [pool_capacity, ...]}
        self.g = [NONE] * self.pool_capacity            # the cost each slot was reached with
        self.key = [0] * self.pool_capacity             # ... and the key of its state
        self.parents = [IDX_NONE] * self.capacity
        self.cursor = 0
        self.goals = []                                 # every goal offer that improved its key: (value, key)
        self.overflowed, self.full = 0, False
        self.iterations = []                            # one record per iteration

    def save(self, rows, slots):
        """slot slots[j] := row j of `rows` (a get_state() dict)."""
        rows = KV._rows(rows)
        if self.rows is None:
            self.rows = {k: np.zeros((self.pool_capacity,) + rows[k].shape[1:], rows[k].dtype) for k in STATE_KEYS}
        for k in STATE_KEYS:
            self.rows[k][np.asarray(slots, np.int64)] = rows[k]

    def keys_of(self, slots):
        from gym_novel_gridworlds_amd.state_keys import keys_of_rows
        return keys_of_rows(KV._rows(self.rows, slots))

    def goal(self):
        """-> (value, {the keys that reached it}) of the cheapest goal, (NONE, set()) while there is none."""
        if not self.goals:
            return NONE, set()
        value = min(v for v, _ in self.goals)
        return value, {k for v, k in self.goals if v == value}

    def start(self, roots):
        """roots: slots, IDX_NONE allowed.  -> best of the roots' offer (value 0, tag ROOT)."""
        roots = [int(r) for r in roots]
        assert len(roots) <= self.capacity
        live = [r for r in roots if r != IDX_NONE]
        keys = np.zeros(len(roots), np.uint64)
        if live:
            keys[[j for j, r in enumerate(roots) if r != IDX_NONE]] = self.keys_of(live)
        _, _, best = self.table.insert_min(keys, [0] * len(roots), [KV.ROOT] * len(roots))
        self.parents = [IDX_NONE] * self.capacity
        for j, r in enumerate(roots):
            if r == IDX_NONE:
                continue
            self.g[r], self.key[r] = self.table.held[int(keys[j])][0], int(keys[j])
            if best[j]:
                self.parents[j] = r
        return best

    def iterate(self):
        """One iteration -> its record: keys uint64 / values / info / best [capacity * A], improved, offered, expanded, overflow, and the
        expand lists."""
        from gym_novel_gridworlds_amd.state_keys import keys_of_rows
        A, cap = self.A, self.capacity
        n = cap * A
        keys, info, values, tags = np.zeros(n, np.uint64), np.zeros(n, np.uint32), [NONE] * n, [KV.ROOT] * n
        live = [j for j in range(cap) if self.parents[j] != IDX_NONE]
        children = None
        if live:                                                                          # step 1: every action's child of every live parent
            slots = np.repeat([self.parents[j] for j in live], A)
            children, reports = XO.oracle_expand(self.spec, self.rows, slots, np.tile(np.arange(A), len(live)))
            children = KV._rows(children)
            at = (np.repeat(live, A) * A + np.tile(np.arange(A), len(live))).astype(np.int64)
            keys[at], info[at] = keys_of_rows(children), reports['info']
            row_of = {int(q): i for i, q in enumerate(at)}
        overflow = 0
        for j in live:                                                                    # step 2: the offers
            p = self.parents[j]
            if self.g[p] == NONE:
                continue
            for a in range(A):
                q = j * A + a
                cost = self.costs[a] if self.costs is not None else self.lut[(int(info[q]) >> 2) & 63]
                total = self.g[p] + cost
                if total >= NONE or total < I32_MIN:
                    overflow += 1
                    continue
                values[q], tags[q] = total, len(self.links) + q
        self.links += [(self.key[self.parents[j]] if self.parents[j] != IDX_NONE else 0, a) for j in range(cap) for a in range(A)]
        _, _, best = self.table.insert_min(keys, values, tags)                            # step 3
        improved = int(best.sum())
        chosen = best.copy()
        for q in np.flatnonzero(best).tolist():                                           # step 4: goals, and what does not go on
            w = int(info[q])
            if (w >> 1) & 1:
                if (w >> 8) & 255 != 14:
                    self.goals.append((values[q], int(keys[q])))
                if self.stop:
                    chosen[q] = False
        if self.keep is None:                                                             # step 5
            first, second, count, full = FO.compact(chosen, A, None, cap)
        else:
            first, second, count = select(values, chosen, self.keep, A, cap)
            full = False
        slots, self.cursor, short = FO.alloc(count[0], self.cursor, self.pool_capacity, cap)
        self.full = self.full or bool(full) or bool(short)
        nxt, pairs = [IDX_NONE] * cap, []                                                 # steps 6 and 7
        for k in range(cap):
            j, a, c = int(first[k]), int(second[k]), int(slots[k])
            if j == IDX_NONE:
                continue
            pairs.append((self.parents[j], a, c))
            if c == IDX_NONE:
                continue
            q = j * A + a
            for name in STATE_KEYS:
                self.rows[name][c] = children[name][row_of[q]]
            self.g[c], self.key[c], nxt[k] = values[q], int(keys[q]), c
        self.parents = nxt
        self.overflowed += overflow
        rec = dict(keys=keys, values=np.array(values, np.int32), info=info, best=best, chosen=chosen, improved=improved,
                   offered=sum(v != NONE for v in values), expanded=sum(c != IDX_NONE for c in nxt), overflow=overflow, pairs=pairs,
                   cursor=self.cursor)
        self.iterations.append(rec)
        return rec
