"""The model of a valued key table (include/ngw.h ngw_key_table_insert_min / _read / _trace): a Python dict from key to (value, tag), fed
one position after the other, and a plain-Python walk of the tags.  `fresh` and `best`, every value and every tag are compared exactly
against it; `where` has no model (tests/key_table_oracle.py WhereBook holds it to its properties).  Nothing here comes from the HIP path."""
import numpy as np

from key_table_oracle import as_u64

NONE = (1 << 31) - 1            # include/ngw.h NGW_VALUE_NONE
ROOT = -1                       # include/ngw.h NGW_TAG_ROOT
IDX_NONE = -(1 << 31)           # include/ngw.h NGW_IDX_NONE


class KeyValueModel:
    """key -> [value, tag] of every key ever stored (NONE / ROOT: never valued).  Key 0 is never stored."""

    def __init__(self):
        self.held = {}
        self.reopened = 0       # improvements of keys that were stored by an EARLIER call

    def __len__(self):
        return len(self.held)

    def insert(self, keys, refused=None):
        """A plain insert: -> (fresh, stored); values and tags stay."""
        n = len(as_u64(keys))
        fresh, stored, _ = self.insert_min(keys, [NONE] * n, None, refused)
        return fresh, stored

    def insert_min(self, keys, values, tags=None, refused=None):
        """-> (fresh, stored, best), bool [count].  The positions run one after the other: a position lowers its key's value when its own is
        strictly smaller than what the key holds at that moment - so among equal values of one call the first position stays -, and the LAST
        position that lowered a key in this call is the call's one improvement of it.  refused[j]: the table turned position j away (it was
        full; which keys it refuses is the table's choice): the position stores and offers nothing."""
        keys = as_u64(keys).tolist()
        values = [int(v) for v in np.asarray(values).tolist()]
        assert len(values) == len(keys) and (tags is None or len(tags) == len(keys))
        fresh, stored, best = np.zeros(len(keys), bool), np.zeros(len(keys), bool), np.zeros(len(keys), bool)
        before = dict((k, v[0]) for k, v in self.held.items())
        last = {}
        for j, k in enumerate(keys):
            if k == 0 or (refused is not None and refused[j]):
                continue
            stored[j] = True
            if k not in self.held:
                self.held[k] = [NONE, ROOT]
                fresh[j] = True
            if values[j] != NONE and values[j] < self.held[k][0]:
                self.held[k][0] = values[j]
                if tags is not None:
                    self.held[k][1] = int(tags[j])
                last[k] = j
        for k, j in last.items():
            best[j] = True
            self.reopened += k in before
        return fresh, stored, best

    def get(self, keys):
        """-> (value, tag) int32 [count]: (NONE, ROOT) for a key that is not held."""
        got = [self.held.get(k, (NONE, ROOT)) for k in as_u64(keys).tolist()]
        return np.array([g[0] for g in got], np.int32).reshape(-1), np.array([g[1] for g in got], np.int32).reshape(-1)


def trace(where, steps, n_actions, tag_of_bucket, buckets):
    """The walk of ngw_key_table_trace: -> (plans int32 [steps, count], length, root int32 [count], bad - F_BAD_INDEX is due).
    tag_of_bucket: {bucket: tag} of the OCCUPIED buckets.  From where[j], follow tag -> bucket tag // n_actions, noting tag % n_actions, until
    a bucket's tag is ROOT; give up - without `bad` - when `steps` links have not reached one."""
    count = len(where)
    plans = np.full((steps, count), -1, np.int32)
    length, root, bad = np.full(count, -1, np.int32), np.full(count, -1, np.int32), False
    for j in range(count):
        b = int(where[j])
        if b == -1 or b == IDX_NONE:
            continue
        acts, ok = [], None
        for _ in range(steps + 1):
            if b < 0 or b >= buckets or b not in tag_of_bucket:
                ok = False
                break
            tg = tag_of_bucket[b]
            if tg == ROOT:
                ok = True
                break
            if len(acts) == steps:
                break
            if tg < 0 or tg >= buckets * n_actions:
                ok = False
                break
            acts.append(tg % n_actions)
            b = tg // n_actions
        if ok is False:
            bad = True
        if ok:
            length[j], root[j] = len(acts), b
            for t, a in enumerate(reversed(acts)):
                plans[t, j] = a
    return plans, length, root, bad


def synthetic_costs(spec):
    """The per-action costs of the label-correcting test: the lowest Left id 1, the lowest Right id 10, every other action 5 - three Lefts (3)
    reach in the third iteration the state one Right (10) reached in the first, so a stored state is reopened by construction."""
    from gym_novel_gridworlds_amd.spec import ACT_LEFT, ACT_RIGHT
    cs = spec.compile()
    kinds = [int(cs.act_kind[a]) for a in range(cs.n_actions)]
    costs = np.full(cs.n_actions, 5, np.int32)
    costs[kinds.index(ACT_LEFT)], costs[kinds.index(ACT_RIGHT)] = 1, 10
    return costs


def _rows(rows, idx=None):
    out = {}
    for k, x in rows.items():
        x = np.asarray(x)
        x = x.reshape(len(x), -1) if k in ('map', 'loc', 'inv') else x
        out[k] = x if idx is None else x[np.asarray(idx, np.int64)]
    return out


def label_correcting(spec, roots, costs, iterations):
    """The search of key_table.py's docstring on the CPU oracle: a generator that yields, first for the roots and then after every
    iteration, (model, keys uint64 [P * A], values int32 [P * A], best bool [P * A]) - P the parents of that iteration, in the order of
    the previous iteration's improved positions; the children of every improved position are the next parents, whatever else they are.
    The model's tags number the entries of model.links = [(parent key, action)], so that chain() can walk them."""
    import expand_oracle as XO
    from gym_novel_gridworlds_amd.state_keys import keys_of_rows
    A = len(costs)
    rows = _rows(roots)
    model = KeyValueModel()
    model.links = []
    keys = keys_of_rows(rows)
    g = np.zeros(len(keys), np.int32)
    _, _, best = model.insert_min(keys, g)
    assert best.all(), "two roots in one state"
    yield model, keys, g, best
    for _ in range(iterations):
        P = len(g)
        children, _ = XO.oracle_expand(spec, rows, np.repeat(np.arange(P), A), np.tile(np.arange(A), P))
        children = _rows(children)
        keys = keys_of_rows(children)
        values = (g[:, None] + costs[None, :]).reshape(-1).astype(np.int32)
        tags = len(model.links) + np.arange(P * A)
        model.links += [(int(pk), a) for pk in keys_of_rows(rows).tolist() for a in range(A)]
        _, _, best = model.insert_min(keys, values, tags)
        yield model, keys, values, best
        take = np.flatnonzero(best)
        rows, g = _rows(children, take), values[take]


def chain(model, key, costs):
    """The way the model's tags lead from a root to `key` (label_correcting's links): -> (root key, [actions in execution order], their cost).
    A stored value is an upper bound of that cost, not always the cost: when a state is reopened, the states that were valued THROUGH it keep
    their values until the search reaches them again, while their chains already run through the cheaper way."""
    acts = []
    while model.held[key][1] != ROOT:
        key, a = model.links[model.held[key][1]]
        acts.append(a)
    return key, acts[::-1], int(sum(int(costs[a]) for a in acts))
