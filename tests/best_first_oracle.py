"""The model of an OPEN-LIST search run (include/ngw.h "an open-list iteration"; gym_novel_gridworlds_amd/search.py open_list=True): steps 0
to 8 with plain Python loops.  Steps 1 to 7 are tests/search_oracle.py's SearchModel with keep=None - the compaction always -, so the
children, the table, the allocation and the statistics come from the CPU oracle as there; the open list is a Python list of f per slot, the
choice a sort of (f, slot), and h the shortest walk of walk.shortest_walk.  Buckets have no model: slot_of_bucket is kept per KEY.  Written
from the contract text and not from search.py, whose numpy references tests/test_best_first_cpu.py holds to a statement of its own.  Nothing
here comes from the HIP path."""
import search_oracle as SX

NONE, IDX_NONE = SX.NONE, SX.IDX_NONE


def heuristic_of(dist, weights, mode):
    """h of one row of walk distances: min / max of weights[k] * dist[k] over weights[k] > 0 and dist[k] >= 0, clamped; 0 where there is none."""
    terms = [int(w) * int(d) for w, d in zip(weights, dist) if int(w) > 0 and int(d) >= 0]
    if not terms:
        return 0
    return min(min(terms) if mode == 'min' else max(terms), NONE - 1)


class BestFirstModel(SX.SearchModel):
    """An open-list search of `capacity` list entries over a pool of `pool_capacity` rows that expands `keep` open states per iteration.
    heuristic: None or (weights, 'min' | 'max')."""

    def __init__(self, spec, capacity, pool_capacity, keep, costs=None, scale=1, stop_at_goals=False, heuristic=None, prune=False):
        super().__init__(spec, capacity, pool_capacity, costs=costs, scale=scale, keep=None, stop_at_goals=stop_at_goals)
        assert 1 <= keep <= capacity and (heuristic is None or heuristic[1] in ('min', 'max'))
        self.k, self.heuristic, self.prune = int(keep), heuristic, bool(prune)
        self.f = [NONE] * self.pool_capacity
        self.h = [0] * self.pool_capacity
        self.slot_of_key = {}                           # the slot that holds the cheapest copy of a state
        self.chosen = [IDX_NONE] * self.capacity        # the slots the last iteration chose ...
        self.expanded_slots = []                        # ... and every slot ever expanded, in order
        self.open_rows = []                             # one record per iteration: chosen, pruned, superseded, open, f_min, f_bound

    def h_of(self, slot):
        if self.heuristic is None:
            return 0
        from gym_novel_gridworlds_amd.walk import shortest_walk
        loc = self.rows['loc'][slot].reshape(-1)
        dist = shortest_walk(self.rows['map'][slot], (int(loc[0]), int(loc[1]), int(self.rows['facing'][slot])), self.spec).dist
        return heuristic_of(dist, self.heuristic[0], self.heuristic[1])

    def open(self, slot):
        self.h[slot] = self.h_of(slot)
        self.f[slot] = min(self.g[slot] + self.h[slot], NONE - 1)

    def start(self, roots):
        best = super().start(roots)
        for j, r in enumerate(int(r) for r in roots):
            if r != IDX_NONE and best[j]:
                self.slot_of_key[self.key[r]] = r
                self.open(r)
        self.parents = [IDX_NONE] * self.capacity       # the first iteration chooses the roots from the list
        return best

    def iterate(self):
        cand = sorted((x, slot) for slot, x in enumerate(self.f) if x != NONE)                 # step 0: SELECT ...
        picked = sorted(slot for _, slot in cand[:self.k])
        goal = self.goal()[0]
        chosen, parents, pruned, old = [IDX_NONE] * self.capacity, [IDX_NONE] * self.capacity, 0, []
        for k, slot in enumerate(picked):                                                      # ... and TAKE
            old.append(self.f[slot])
            self.f[slot] = NONE
            chosen[k] = parents[k] = slot
            if self.prune and old[-1] >= goal:
                parents[k], pruned = IDX_NONE, pruned + 1
        self.chosen, self.parents = chosen, parents
        self.expanded_slots += [p for p in parents if p != IDX_NONE]
        rec = super().iterate()                                                                # steps 1 to 7: self.parents are the children now
        superseded = 0
        for c in self.parents:                                                                 # step 6's superseding
            if c == IDX_NONE:
                continue
            earlier = self.slot_of_key.get(self.key[c])
            if earlier is not None and earlier != c:
                self.f[earlier] = NONE
                superseded += 1
            self.slot_of_key[self.key[c]] = c
        for c in self.parents:                                                                 # step 8
            if c != IDX_NONE:
                self.open(c)
        self.open_rows.append(dict(chosen=len(picked), pruned=pruned, superseded=superseded, open=len(cand), f_min=min(old) if old else NONE,
                                   f_bound=max(old) if old else NONE))
        rec.update(self.open_rows[-1])
        return rec

    def proven(self):
        goal = self.goal()[0]
        if goal == NONE or not self.open_rows:
            return False
        return self.open_rows[-1]['open'] == 0 or self.open_rows[-1]['f_min'] >= goal
