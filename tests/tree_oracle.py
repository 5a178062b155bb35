"""A plain-Python model of TreeSearch (gym_novel_gridworlds_amd/tree.py) on the unmodified CPU oracle: the table is a DICT from key to the
node's statistics - which bucket a key gets is not part of the table's contract, so the device is compared THROUGH THE KEYS (assert_tree below:
visits / returns / mask words / rows gathered at table.lookup(key) for every key the model holds, and len(table) against the model's size).
An iteration's playout is guided_playout_oracle.oracle_guided - the forward simulation on the oracle's step, mask, key and the public choice
rule -; the leaf, the backup and the rows are written out here on the dict, not through tree.py's array references (test_tree_search_cpu.py
holds the two to each other)."""
import numpy as np

import expand_oracle as XO
import guided_playout_oracle as GO
import pairs_oracle as PA
import trajectory_oracle as TO
from gym_novel_gridworlds_amd.spec import IDX_NONE
from gym_novel_gridworlds_amd.state_keys import KEY_STATE, keys_of_rows
from gym_novel_gridworlds_amd.tree import puct_rows_reference


class Node:
    def __init__(self, A):
        self.n, self.w = np.zeros(A, np.int32), np.zeros(A, np.int64)
        self.mask, self.row, self.p = np.uint64(0), np.zeros(A, np.float32), np.zeros(A, np.float32)


class TreeModel:
    """rows: the states the roots index (a get_state()-style dict or an oracle State).  buckets: how many keys the table holds before it
    refuses (KeyTable.buckets).  priors: None, or a function key -> float32 [A]; a node's priors are ZERO until fill_priors() writes them, as
    the device's tensor is until the caller fills it."""

    def __init__(self, spec, rows, playouts, steps, c, q_init=0.0, weights=None, fields=KEY_STATE, buckets=1 << 30, priors=None, autoreset=False, horizon=0):
        self.spec, self.rows, self.playouts, self.steps, self.c, self.q_init = spec, rows, int(playouts), int(steps), c, q_init
        self.weights, self.fields, self.buckets, self.priors, self.auto, self.horizon = weights, fields, buckets, priors, autoreset, horizon
        self.A = spec.compile().n_actions
        self.clear()

    def clear(self):
        self.node, self.it, self.roots, self.full, self.bad, self.report, self.last = {}, 0, np.zeros(0, np.int64), False, False, [], None

    def __len__(self):
        return len(self.node)

    def fill_priors(self):
        for k, nd in self.node.items():
            nd.p = np.asarray(self.priors(k), np.float32)

    def reweight(self, keys):
        for k in keys:
            nd = self.node[k]
            rows, bad = puct_rows_reference(nd.n[None], nd.w[None], np.array([nd.mask], np.uint64), self.c, self.q_init, None if self.priors is None else nd.p[None])
            nd.row, self.bad = rows[0], self.bad or bad

    def insert(self, keys):
        """table.insert of one call's keys -> accepted bool per key.  A call that would leave the table between full and not full - more new keys
        than free buckets, but some free - has no deterministic answer on the device: the tests avoid it, the model refuses to guess."""
        new = []
        for k in keys:
            if k and k not in self.node and k not in new:
                new.append(k)
        free = self.buckets - len(self.node)
        assert len(new) <= free or free == 0, "which of %d new keys get the last %d buckets is not defined" % (len(new), free)
        ok = free > 0 or not new
        if not ok:
            self.full = True
        for k in (new if ok else ()):
            self.node[k] = Node(self.A)
        return [bool(k) and k in self.node for k in keys], len(new) if ok else 0

    def n_rows(self):
        r = self.rows
        return len(r['facing'] if isinstance(r, dict) else r.facing)

    def start(self, roots, rows=None):
        if rows is not None:
            self.rows = rows
        roots = np.asarray(roots, np.int64)
        self.roots = roots
        live = (roots >= 0) & (roots < self.n_rows())
        at = np.nonzero(live)[0]
        if not len(at):
            return
        now = PA.rows_of(XO.rows_state(self.spec, self.rows, roots[at]))
        keys = keys_of_rows(now, self.fields).tolist()
        masks = TO.mask_words(self.spec, {k: now[k] for k in PA.STATE_KEYS})
        held, _ = self.insert(keys)
        for k, m, h in zip(keys, masks.tolist(), held):
            if h:
                self.node[k].mask = np.uint64(m)
        self.reweight(sorted({k for k, h in zip(keys, held) if h}))

    def playout(self, seed):
        """The guided playout of iteration self.it -> oracle_guided's dict with a 'live' mask; a root that is IDX_NONE or out of range is run from
        row 0 and then blanked (a pair's playout does not depend on the other pairs)."""
        roots = self.roots
        live = (roots >= 0) & (roots < self.n_rows())
        e = GO.oracle_guided(self.spec, self.rows, np.where(live, roots, 0), self.steps, seed, np.array(list(self.node), np.uint64),
                             lambda k: self.node[int(k)].row, self.weights, self.it * self.playouts, self.auto, self.horizon, self.fields)
        e['live'] = live
        for name in ('actions', 'keys', 'rewards', 'masks', 'before', 'hit'):
            e[name] = np.asarray(e[name]).copy()
        e['actions'][:, ~live] = -1
        for name in ('keys', 'rewards', 'masks', 'before', 'hit'):
            e[name][:, ~live] = 0
        e['depth'] = np.where(live, e['depth'], 0).astype(np.int32)
        e['length'] = np.where(live, e['reports']['length'], 0).astype(np.int32)
        return e

    def run(self, iterations, seed, bootstrap=None):
        for _ in range(iterations):
            self.iterate(self.playout(seed), bootstrap)

    def iterate(self, e, bootstrap=None, grow=True):
        """Steps 2 to 5 on the dict.  grow=False: no pair has a leaf (a backup without a grow)."""
        depth, length, count = e['depth'], e['length'], len(e['depth'])
        leaf = [0] * count
        for j in range(count):
            d = int(depth[j])
            if grow and 1 <= d < int(length[j]):
                leaf[j] = int(e['keys'][d - 1, j])
        held, grown = self.insert(leaf)
        for j in range(count):
            if held[j]:
                self.node[leaf[j]].mask = np.uint64(e['masks'][int(depth[j]), j])
        touched, backed = set(), 0
        for j in range(count):
            d = int(depth[j])
            if d < 1:
                continue
            for t in range(min(d, int(length[j]) - 1), -1, -1):
                k = int(e['before'][t, j]) if t < d else (leaf[j] if held[j] else 0)
                if not k:
                    continue
                G = int(e['rewards'][t:, j].sum()) + (0 if bootstrap is None else int(bootstrap[j]))
                nd, a = self.node[k], int(e['actions'][t, j])
                nd.n[a] += 1
                nd.w[a] += G
                touched.add(k)
                backed += 1
        self.reweight(sorted(touched | {leaf[j] for j in range(count) if held[j]}))
        self.report.append((int((length >= 1).sum()), grown, sum(1 for j in range(count) if leaf[j] and not held[j]), backed, int(depth.max()) if count else 0))
        e['leaf'], e['held'] = np.array(leaf, np.uint64), np.array(held, bool)
        self.last = e
        self.it += 1

    def best_actions(self, keys):
        out = []
        for k in keys:
            nd = self.node.get(int(k))
            valid = [a for a in range(self.A) if nd is not None and (int(nd.mask) >> a) & 1]
            out.append(max(valid, key=lambda a: (nd.n[a], -a)) if valid else -1)
        return np.array(out, np.int32)


def assert_tree(t, table, m, where, flags=None):
    """The device tree `t` against the model `m`, through the keys: everything the model holds is found in the table, with equal bytes."""
    keys = np.array(list(m.node), np.uint64)
    assert len(table) == len(m), "%s: the table holds %d keys, the model %d" % (where, len(table), len(m))
    if len(keys):
        b = table.lookup(keys)
        assert (b >= 0).all(), "%s: %d of the model's keys are not in the table" % (where, int((b < 0).sum()))
        assert len(set(b.tolist())) == len(b)
        got = dict(n=t.visits.cpu().numpy()[b], w=t.returns.cpu().numpy()[b], mask=t.mask_words.cpu().numpy().view(np.uint64)[b],
                   row=t.rows.cpu().numpy().view(np.uint32)[b])
        exp = dict(n=np.stack([nd.n for nd in m.node.values()]), w=np.stack([nd.w for nd in m.node.values()]),
                   mask=np.array([nd.mask for nd in m.node.values()], np.uint64), row=np.stack([nd.row for nd in m.node.values()]).view(np.uint32))
        for name in ('mask', 'n', 'w', 'row'):
            bad = np.argwhere(got[name] != exp[name])
            assert not len(bad), "%s: %s differs at %d places, first %s: got %s expected %s" % (
                where, name, len(bad), tuple(bad[0]), got[name][tuple(bad[0])], exp[name][tuple(bad[0])])
        # every other bucket is untouched: zero statistics, a zero row
        rest = np.ones(table.buckets, bool)
        rest[b] = False
        assert not t.visits.cpu().numpy()[rest].any() and not t.returns.cpu().numpy()[rest].any() and not t.rows.cpu().numpy()[rest].any(), where
    st = t.stats()
    assert st.iterations == m.it, (where, st.iterations, m.it)
    rows = np.array(m.report[-64:], np.int64).reshape(-1, 5)
    got = np.stack([st.alive, st.grown, st.refused, st.backed_up, st.depth], 1).astype(np.int64)
    assert (got == rows).all(), "%s: the report differs:\n%s\n%s" % (where, got, rows)
    if flags is not None:
        assert st.flags == flags, "%s: flags %d, expected %d" % (where, st.flags, flags)
    return st
