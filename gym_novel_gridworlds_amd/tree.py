"""Device-side tree-search runs of a Snapshot: whole MCTS iterations - descend, simulate, expand one node, back up, reweight - over one key
table, enqueued from ONE call with no host wait and no torch operation in between (include/ngw.h ngw_tree_*; the kernels are
csrc/ngw_tree.inc, the driver csrc/ngw_abi_tree.cpp).  The Monte-Carlo twin of search.py.

    table = env.key_table(1 << 16)
    t = pool.tree_search(table, playouts=4096, steps=32, c=1.5)
    t.start(roots)                                        # the roots' keys inserted, their mask words learned, their rows written
    t.run(64, seed)                                       # sixty-four iterations, enqueued; returns at once
    a = t.best_actions(roots)                             # the most-visited valid action of each root (the caller's host wait)

One iteration is the loop README's "Guided playouts" spells out - playout(table=, table_weights=t.rows), tree_steps, index_add_ on N and Q,
table.insert of the new leaves, the rows recomputed - with three differences that the host loop cannot have.  The rows are recomputed UNDER
THE VALID-ACTION MASK of each node (the word the playout's own draw at that state was made under, kept per bucket in t.mask_words), so an
argmax never lands on an action the state refuses and a node never falls back to uniform play for that reason.  The statistics are INTEGERS
(t.visits int32, t.returns int64), so a backup is a set of integer additions and its bytes do not depend on the order the device runs them
in - a float index_add_ does.  And nothing between the launches runs on the host.  The rule of a row is PUCT with a one-hot result:

    q[a] = returns[b, a] / visits[b, a]  (q_init where visits is 0)      u[a] = c * p[a] * sqrt(n_b + 1) / (1 + visits[b, a])

in binary32, every operation rounded on its own (puct_rows_reference states the order), p the caller's priors (priors=True: t.priors, filled
by the caller from its policy network, indexed by bucket) or 1; the row is 1.0 at the valid action of the largest q + u, the lowest id on
ties, and 0.0 elsewhere - the weighted rule of the guided playout then picks that action with certainty, for every Philox word: in
sample.choose_weighted a one-hot row has mass 1, thr = u * 1 < 1 = c[a], every action before a has v = 0, and in the corner w = 0 (thr = 0)
the comparison c[a] > thr is strict and still holds.  A bucket whose mask word is 0 (never learned) has an all-zero row: the uniform rule.

The stages are callable on their own, for a loop that asks a value network between them:

    r = pool.playout(roots, T, seed, first_pair=i * n, record=True, path_keys=True, rewards=True, masks=True, table=table, table_weights=t.rows,
                     device=True)
    t.grow(r)                                             # the leaves: leaf -> table.insert -> mask words; t.where_leaf names their buckets
    v = value_net(...)                                    # int32 [count]: the value of each pair's leaf, in reward units (0 where it has none)
    t.backup(r, bootstrap=v)                              # G_t = the rewards from t on + v
    t.reweight()                                          # the rows of every bucket that backup touched

With spread=S (1 to 64) a row is not one-hot: it is the allotment k[a] that S successive PUCT choices with virtual visits make - the divisor of
u grows with every choice an action received, sqrt(n_b + 1 + i) with the round i, q does not change - and every pair draws its own action from
it by (seed, pair, t), so the pairs of one root spread inside the tree and one iteration grows several nodes per root state.  With discount=d
the backup is G_t = r_t + D(G_{t+1}), D(x) = (round(d * 65536) * x) >> 16 in int64: integers still, so the bytes stay independent of order.

leaf_reference, backup_reference, puct_rows_reference, spread_rows_reference and iteration_reference state the contract in numpy.  NOT built:
virtual loss through atomics, max-backups, a tree across ranks, hipGraph capture, and the leaf's observation for a network - the caller gets it from
snap.lidar_observation after replaying the recorded actions with limits=depth.

A tree search is rank-local, as a search is: under ShardedVecNovelGridworld it belongs to the local env's pool and table."""
import collections
import ctypes as C

import numpy as np

from . import _cabi

WEIGHT_MIN, WEIGHT_MAX = np.float32(2.0 ** -64), np.float32(2.0 ** 64)      # the bounds of a cleaned prior (sample.py's)
STATS_ROWS = _cabi.TREE_ROWS
MAX_ENTRIES = (1 << 31) - 1

TreeStats = collections.namedtuple('TreeStats', 'where n w mask')
TreeReport = collections.namedtuple('TreeReport', 'iterations alive grown refused backed_up depth flags')


def leaf_reference(depth, length, keys, masks):
    """Step 2 in numpy -> (leaf_keys uint64 [count], leaf_masks uint64 [count]).  depth, length int32 [count]; keys, masks uint64 [T, count] as a
    guided playout records them.  Pair j with 1 <= depth[j] < length[j]: keys[depth[j] - 1, j] - the first state the table does not hold - and
    masks[depth[j], j]; every other pair: 0, 0."""
    depth, length = np.asarray(depth, np.int64), np.asarray(length, np.int64)
    keys, masks = np.asarray(keys).view(np.uint64), np.asarray(masks).view(np.uint64)
    lk, lm = np.zeros(len(depth), np.uint64), np.zeros(len(depth), np.uint64)
    for j in np.flatnonzero((depth >= 1) & (depth < length)).tolist():
        lk[j], lm[j] = keys[depth[j] - 1, j], masks[depth[j], j]
    return lk, lm


def discount_reference(x, g):
    """D of rule 4 on a Python int in int64 range -> a Python int: x itself for g == 65536, else (g * x) >> 16 - the product wrapped to int64, the
    shift arithmetic (floor)."""
    if g == 65536:
        return x
    y = (g * x) & 0xFFFFFFFFFFFFFFFF
    return (y - (1 << 64) if y >> 63 else y) >> 16


def backup_reference(visits, returns, actions, rewards, where, depth, length, where_leaf=None, bootstrap=None, discount_q16=65536):
    """Step 4 in numpy: visits int32 [buckets, A] and returns int64 [buckets, A] updated in place -> touched int32 [T, count], the bucket of
    every step that was backed up, -1 elsewhere.  actions, rewards, where int32 [T, count]; depth, length int32 [count]; where_leaf int32
    [count] or None (no pair has a leaf); bootstrap int32 [count] or None.  Pair j with d = depth[j] >= 1, for t from min(d, length[j] - 1)
    down to 0: e = where[t, j] for t < d, where_leaf[j] for t == d; where e is a bucket and actions[t, j] an action: visits[e, a] += 1,
    returns[e, a] += G_t = rewards[t:, j].sum() + bootstrap[j], wrapping as int32 / int64 do.  discount_q16 = g below 65536 (ngw_tree_set_rule):
    with n = length[j] clamped to [0, T], G_n = bootstrap[j] + rewards[n:, j].sum() (a playout records 0 there) and G_t = rewards[t, j] +
    ((g * G_{t+1}) >> 16) for t < n - discount_reference; the bootstrap is discounted n times, not T."""
    g = int(discount_q16)
    if not 0 <= g <= 65536:
        raise ValueError("discount_q16: %r outside [0, 65536]" % (discount_q16,))
    actions, rewards, where = np.asarray(actions), np.asarray(rewards, np.int64), np.asarray(where)
    T, count = actions.shape
    buckets, A = visits.shape
    touched = np.full((T, count), -1, np.int32)
    v, r = visits.reshape(-1).view(np.uint32), returns.reshape(-1).view(np.uint64)
    for j in range(count):
        d, n = int(depth[j]), min(max(int(length[j]), 0), T)
        if d < 1:
            continue
        boot = int(0 if bootstrap is None else bootstrap[j])
        Gs = [0] * n + [boot + int(rewards[n:, j].sum())]                       # G_t of the executed steps, G_n behind them
        for t in range(n - 1, -1, -1):
            y = (int(rewards[t, j]) + discount_reference(Gs[t + 1], g)) & 0xFFFFFFFFFFFFFFFF
            Gs[t] = y - (1 << 64) if y >> 63 else y
        for t in range(min(d, n - 1), -1, -1):
            G = Gs[t]
            e = int(where[t, j]) if t < d else (-1 if where_leaf is None else int(where_leaf[j]))
            a = int(actions[t, j])
            if 0 <= e < buckets and 0 <= a < A:
                v[e * A + a] = (int(v[e * A + a]) + 1) & 0xFFFFFFFF
                r[e * A + a] = (int(r[e * A + a]) + G) & 0xFFFFFFFFFFFFFFFF
                touched[t, j] = e
    return touched


def puct_rows_reference(visits, returns, mask_words, c, q_init, priors=None):
    """Step 5 in numpy, for n rows -> (rows float32 [n, A], bad: a prior raised F_BAD_WEIGHT).  visits int32 [n, A], returns int64 [n, A],
    mask_words uint64 [n], priors float32 [n, A] or None.  Every operation is one rounded binary32 operation, in this order:
        q = float32(returns) / float32(visits) where visits > 0, else q_init;  u = ((c * p) * sqrt(float32(n_b + 1))) / float32(1 + visits)
    with n_b the row's visit sum in 64 bits and p the cleaned prior (outside [2^-64, 2^64]: 0) or 1; the row is 1.0 at the pick of: for a in
    order, bit a of the mask set and (no pick yet or q[a] + u[a] > the pick's) - and 0.0 elsewhere, all 0.0 for mask 0."""
    visits, returns = np.asarray(visits, np.int64), np.asarray(returns, np.int64)
    m = np.asarray(mask_words).view(np.uint64).reshape(-1)
    n, A = visits.shape
    f32 = np.float32
    bad = False
    with np.errstate(all='ignore'):
        if priors is None:
            p = np.ones((n, A), f32)
        else:
            x = np.asarray(priors, f32)
            bad = bool((~((x >= 0) & (x <= WEIGHT_MAX))).any())
            p = np.where((x >= WEIGHT_MIN) & (x <= WEIGHT_MAX), x, f32(0)).astype(f32)
        root = np.sqrt((visits.sum(1) + 1).astype(f32)).astype(f32)
        q = np.where(visits > 0, returns.astype(f32) / np.where(visits > 0, visits, 1).astype(f32), f32(q_init)).astype(f32)
        u = (((f32(c) * p).astype(f32) * root[:, None]).astype(f32) / (1 + visits).astype(f32)).astype(f32)
        score = (q + u).astype(f32)
    rows = np.zeros((n, A), f32)
    for i in range(n):
        pick = -1
        for a in range(A):
            if (int(m[i]) >> a) & 1 and (pick < 0 or score[i, a] > score[i, pick]):
                pick = a
        if pick >= 0:
            rows[i, pick] = 1.0
    return rows, bad


def spread_rows_reference(visits, returns, mask_words, c, q_init, spread, priors=None):
    """Step 5 under ngw_tree_set_rule's spread = S in [1, 64], for n rows -> (rows float32 [n, A], bad).  The arguments and the cleaning of the
    priors are puct_rows_reference's.  Per row with a mask word that is not 0: k = 0; for i in 0 .. S-1: the scores of puct_rows_reference with
    sqrt(float32(n_b + 1 + i)) and the divisor float32(1 + visits + k) - the integers summed in 64 bits, then rounded once -, its ordered walk's
    pick, k[pick] += 1; the row is float32(k).  S = 1: puct_rows_reference's bytes."""
    S = int(spread)
    if not 1 <= S <= 64:
        raise ValueError("spread: %r outside [1, 64]" % (spread,))
    visits, returns = np.asarray(visits, np.int64), np.asarray(returns, np.int64)
    m = np.asarray(mask_words).view(np.uint64).reshape(-1)
    n, A = visits.shape
    f32 = np.float32
    bad = False
    rows = np.zeros((n, A), f32)
    with np.errstate(all='ignore'):
        if priors is None:
            p = np.ones((n, A), f32)
        else:
            x = np.asarray(priors, f32)
            bad = bool((~((x >= 0) & (x <= WEIGHT_MAX))).any())
            p = np.where((x >= WEIGHT_MIN) & (x <= WEIGHT_MAX), x, f32(0)).astype(f32)
        total = visits.sum(1)
        q = np.where(visits > 0, returns.astype(f32) / np.where(visits > 0, visits, 1).astype(f32), f32(q_init)).astype(f32)
        cp = (f32(c) * p).astype(f32)
        for i in range(n):
            valid = [a for a in range(A) if (int(m[i]) >> a) & 1]
            if not valid:
                continue
            k = np.zeros(A, np.int64)
            for r in range(S):
                root = np.sqrt(f32(int(total[i]) + 1 + r)).astype(f32)
                score = (q[i] + ((cp[i] * root).astype(f32) / (1 + visits[i] + k).astype(f32)).astype(f32)).astype(f32)
                pick = -1
                for a in valid:
                    if pick < 0 or score[a] > score[pick]:
                        pick = a
                k[pick] += 1
            rows[i] = k.astype(f32)
    return rows, bad


def iteration_reference(visits, returns, mask_words, rows, actions, rewards, where, depth, length, keys, masks, where_leaf, c, q_init, priors=None,
                        bootstrap=None, spread=1, discount_q16=65536):
    """One iteration of TreeSearch.run behind its playout, in numpy: steps 2 to 5 of include/ngw.h's ngw_tree_run.  visits, returns, mask_words
    and rows ([buckets, A], [buckets]) are updated in place; the recorded arrays are the playout's; where_leaf int32 [count]: the bucket the
    table gives each leaf key (-1: key 0 or refused - which bucket a key gets is the table's choice, so it is an input here, as `where` is
    in search.relax_reference); spread, discount_q16: the rule of ngw_tree_set_rule (the defaults: today's iteration).
    -> (leaf_keys, leaf_masks, touched, bad)."""
    lk, lm = leaf_reference(depth, length, keys, masks)
    where_leaf = np.asarray(where_leaf, np.int64)
    for j in np.flatnonzero((where_leaf >= 0) & (lm != 0)).tolist():
        mask_words[where_leaf[j]] = lm[j]
    touched = backup_reference(visits, returns, actions, rewards, where, depth, length, where_leaf, bootstrap, discount_q16)
    b = np.unique(touched[touched >= 0])
    bad = False
    if len(b):
        rows[b], bad = spread_rows_reference(visits[b], returns[b], mask_words[b], c, q_init, spread, None if priors is None else priors[b])
    return lk, lm, touched, bad


def best_actions_reference(visits, mask_words):
    """TreeSearch.best_actions in numpy: per row the most-visited action among the bits of its mask word, the lowest id on ties; -1 for mask 0."""
    visits, m = np.asarray(visits, np.int64), np.asarray(mask_words).view(np.uint64).reshape(-1)
    out = np.full(len(m), -1, np.int32)
    for i in range(len(m)):
        for a in range(visits.shape[1]):
            if (int(m[i]) >> a) & 1 and (out[i] < 0 or visits[i, a] > visits[i, out[i]]):
                out[i] = a
    return out


class TreeSearch:
    """Whole MCTS iterations over one KeyTable, rooted in slots of a Snapshot or in the envs' current states (Snapshot.tree_search).  It owns, in
    the env's device memory: `visits` int32 [buckets, A], `returns` int64 [buckets, A], `mask_words` int64 [buckets] (the uint64 valid-action
    word of the state in each bucket, 0: never learned), `rows` float32 [buckets, A] (what its guided playouts read as table_weights),
    `priors` float32 [buckets, A] with priors=True (zero until the caller fills them), and the recorded arrays of the last iteration's playout
    (`last`: actions, keys, rewards, masks, where [T, playouts]; depth, length, ret, ended, info [playouts]; leaf_keys, leaf_masks, where_leaf,
    fresh [playouts]; touched [T, playouts]).  The tensors are views of the library's ONE allocation: gone with close(), the snapshot, the table
    or the env.  run() allocates nothing.  start(), run() and the stages are enqueued on the env's stream and return at once; read(),
    best_actions() and stats() wait (read / best_actions with device=True do not).
    playouts: the capacity in pairs per iteration; steps: T, fixed here.  c, q_init: the PUCT rule's (module docstring).  weights: None or float32
    [A], the default policy of a state outside the table (the heavy playout's weights).  fields: the KEY_* selection of a node.
    plain_backup=True: the backup adds lane by lane instead of combining inside the wave - the same bytes, for A/B timing.
    spread: S in [1, 64] - a row is the allotment of S successive PUCT choices with virtual visits (spread_rows_reference), so the pairs of one
    root spread over up to S actions at every node and an iteration grows more than one node per root state; `spread` holds it.  discount: a
    float in [0, 1], applied in integers as discount_q16 = round(discount * 65536) per executed step (backup_reference); 1.0: none.
    clear() empties the table AND the statistics; table.clear() alone does not touch the statistics - the rows then describe keys that are gone."""

    def __init__(self, snap, table, playouts, steps, c=1.0, q_init=0.0, priors=False, weights=None, fields=None, plain_backup=False, spread=1, discount=1.0,
                 rows16=0):
        import torch
        from .snapshot import MapsTooLarge
        from .state_keys import KEY_STATE, check_fields
        from .vec_env import _DevArray
        self.snap, self.env, self.table = snap, snap.env, table
        snap._open()
        if not hasattr(table, '_open_for'):
            raise ValueError("table: a KeyTable expected")
        table._open_for(self.env)
        A = self.env.n_actions
        for name, v in (('playouts', playouts), ('steps', steps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("%s: an integer >= 1 expected, got %r" % (name, v))
        self.playouts, self.steps = int(playouts), int(steps)
        if self.playouts * self.steps > MAX_ENTRIES:
            raise ValueError("playouts * steps = %d * %d recorded entries per iteration (at most 2^31 - 1)" % (self.playouts, self.steps))
        if table.buckets * A > MAX_ENTRIES:
            raise ValueError("buckets * n_actions = %d entries of statistics (at most 2^31 - 1)" % (table.buckets * A))
        if isinstance(fields, (int, np.integer)) and not isinstance(fields, bool) and int(fields) == 0:
            raise ValueError("fields == 0: a node needs a non-empty selection of KEY_* bits")
        self.fields = check_fields(KEY_STATE if fields is None else fields)
        self.c, self.q_init = float(c), float(q_init)
        if not (np.isfinite(np.float32(self.c)) and np.isfinite(np.float32(self.q_init))):
            raise ValueError("c = %r, q_init = %r: finite float32 values expected" % (c, q_init))
        if weights is not None:
            if hasattr(weights, 'data_ptr'):
                weights = weights.cpu().numpy()
            weights = np.ascontiguousarray(weights, np.float32)
            if weights.shape != (A,):
                raise ValueError("weights: float32 [%d] expected, got shape %s" % (A, list(weights.shape)))
        self.weights = weights
        if isinstance(spread, bool) or not isinstance(spread, (int, np.integer)) or not 1 <= spread <= 64:
            raise ValueError("spread: an integer in [1, 64] expected, got %r" % (spread,))
        if isinstance(discount, bool) or not isinstance(discount, (int, float, np.integer, np.floating)) or not 0.0 <= float(discount) <= 1.0:
            raise ValueError("discount: a number in [0, 1] expected, got %r" % (discount,))
        if isinstance(rows16, bool) or rows16 not in (0, 1, 2) or (rows16 == 2 and spread > 1):
            raise ValueError("rows16: 0, 1 or 2 expected (2, the one-lane reweight, with spread = 1 only), got %r with spread = %d" % (rows16, spread))
        self.spread, self.discount_q16, self._rows16 = int(spread), int(round(float(discount) * 65536)), int(rows16)
        self._t, self._keep, self._grown = C.c_void_p(), None, None
        opt = _cabi.TreeOptions(self.playouts, self.steps, self.fields, self.c, self.q_init, int(bool(priors)), int(bool(plain_backup)), _cabi._ptr(weights, np.float32))
        try:
            _cabi.check(_cabi.lib().ngw_tree_create(self.env._h, table._t, C.byref(opt), C.byref(self._t)))
        except ValueError as e:
            if str(e).startswith('map_size'):
                raise MapsTooLarge(str(e)) from None
            raise
        if (self.spread, self.discount_q16, self._rows16) != (1, 65536, 0):       # (a default tree makes the calls it always made)
            rule = _cabi.TreeRule(self.spread, self.discount_q16, self._rows16, 0)
            try:
                _cabi.check(_cabi.lib().ngw_tree_set_rule(self.env._h, self._t, C.byref(rule)))
            except Exception:
                _cabi.lib().ngw_tree_destroy(self.env._h, self._t)
                raise
        arr = _cabi.TreeArrays()
        _cabi.check(_cabi.lib().ngw_tree_arrays(self.env._h, self._t, C.byref(arr)))
        dev = 'cuda:%d' % self.env.device
        self._dev = torch.device(dev)
        B, P, T = int(table.buckets), self.playouts, self.steps
        view = lambda name, shape, typ: torch.as_tensor(_DevArray(getattr(arr, name), shape, typ), device=dev)   # noqa: E731
        self.visits, self.returns = view('visits', (B, A), '<i4'), view('returns', (B, A), '<i8')
        self.mask_words, self.rows = view('mask_words', (B,), '<i8'), view('rows', (B, A), '<f4')
        self.priors = view('priors', (B, A), '<f4') if priors else None
        self.roots = view('roots', (P,), '<i4')
        step = {k: view(k, (T, P), typ) for k, typ in (('actions', '<i4'), ('keys', '<i8'), ('rewards', '<i4'), ('masks', '<i8'), ('where', '<i4'), ('touched', '<i4'))}
        pair = {k: view(k, (P,), typ) for k, typ in (('depth', '<i4'), ('length', '<i4'), ('ret', '<i4'), ('ended', '|u1'), ('info', '<i4'), ('leaf_keys', '<i8'),
                                                     ('leaf_masks', '<i8'), ('where_leaf', '<i4'), ('fresh', '|u1'))}
        self.last = dict(step, **pair)
        self.where_leaf = self.last['where_leaf']
        self.n_actions = A

    def _open(self):
        if not self._t:
            raise ValueError("tree search is closed")
        self.snap._open()
        self.table._open_for(self.env)
        return self._t

    def _enqueue(self, call, uploaded=()):
        from .snapshot import enqueue_ordered
        enqueue_ordered(self.env, self, call, 1, list(uploaded), True)
        self._keep = None                       # (as in Search._enqueue: an uploaded list is ordered by torch's allocator)

    def start(self, roots, from_envs=False, source=None):
        """The roots of the trees: slots of `source` (another Snapshot of the same env; default: the pool this object was made from) or, with
        from_envs=True, env indices - one tree per env, all in the one table.  A list / numpy array (checked; IDX_NONE is allowed and skipped)
        or a contiguous torch int32 tensor on the env's device, used in place; at most `playouts`, and the later iterations run one pair per
        root.  Their keys are inserted, their mask words learned and their rows written; visits and returns of a state the table already
        held are KEPT, so calling start() again after a committed step re-roots the trees and keeps what was learned below the new roots.
        Enqueued; no host wait."""
        from .search import check_roots
        from .snapshot import tensor_len, upload
        t = self._open()
        src, n_rows, _ = self.snap._source(source, from_envs, 'tree_search')
        r, count = check_roots(roots, n_rows, self.playouts, lambda x: tensor_len(self._dev, 'roots', x))
        (ptr,), uploaded = upload(self._dev, count, r)
        h, L = self.env._h, _cabi.lib()
        self._grown = None
        self._enqueue(lambda: L.ngw_tree_start(h, t, src, ptr, count), uploaded)

    def run(self, iterations, seed):
        """`iterations` whole iterations under `seed`, enqueued on the env's stream; returns at once.  Iteration number i (counted since
        creation or clear()) draws pair j as global pair i * playouts + j of the seed's stream, so run(4, seed) and four run(1, seed) leave
        identical statistics for every key (identical bytes wherever the table gives the keys the same buckets)."""
        t = self._open()
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= MAX_ENTRIES:
            raise ValueError("iterations: an integer in [0, 2^31 - 1] expected, got %r" % (iterations,))
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed: %d outside [0, 2^64)" % seed)
        h, L = self.env._h, _cabi.lib()
        self._grown = None
        self._enqueue(lambda: L.ngw_tree_run(h, t, int(iterations), seed))

    # ------------------------------------------------------------------ the stages on their own
    def _recorded(self, result, names):
        """The named per-step fields of a guided playout's result as contiguous device tensors [T, count] (+ depth, length) -> (tensors, T, count)."""
        import torch
        out = []
        depth = result.depth
        count = int(np.prod(tuple(depth.shape))) if len(tuple(depth.shape)) else 1
        for name in names + ('depth', 'length'):
            x = getattr(result, name)
            if x is None:
                raise ValueError("the result holds no %s (playout(..., record=True, path_keys=True, rewards=True, masks=True, table=...) records them)" % name)
            if not isinstance(x, torch.Tensor):
                x = np.asarray(x)
                x = torch.from_numpy(np.ascontiguousarray(x.view(np.int64) if x.dtype == np.uint64 else x))
            want = torch.int64 if name in ('keys', 'masks') else torch.int32
            x = x.to(self._dev).to(want).contiguous()
            out.append(x)
        T = int(out[0].shape[0]) if names else self.steps
        if count > self.playouts or not 1 <= T <= self.steps:
            raise ValueError("a result of %d pairs and %d steps in a tree search of %d playouts and %d steps" % (count, T, self.playouts, self.steps))
        return out, T, count

    def grow(self, result):
        """Steps 2 and 3 for a guided playout's `result` (path_keys=True, masks=True): the leaf of every pair - the first state it reached
        that the table does not hold - is inserted and its mask word stored; `where_leaf` (int32 [playouts], -1: none) names the buckets.
        The statistics of the new buckets are zero.  Enqueued; no host wait."""
        t = self._open()
        (keys, masks, depth, length), T, count = self._recorded(result, ('keys', 'masks'))
        p = [C.c_void_p(x.data_ptr()) for x in (depth, length, keys, masks)]
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda: L.ngw_tree_grow(h, t, *p, count, count, T), [keys, masks, depth, length])
        self._grown = result

    def backup(self, result, bootstrap=None):
        """Step 4 for a guided playout's `result` (record=True, rewards=True): every executed step inside the tree adds 1 to visits and its
        return-to-go to returns; the step AT the leaf counts where grow(result) ran before (the same result object), otherwise no pair has a
        leaf.  bootstrap: None or int32 [count] - a list / numpy array or a device tensor -, added to every return of its pair: the value of
        the pair's leaf in reward units (0 where it has none).  Enqueued; no host wait."""
        import torch
        t = self._open()
        (actions, rewards, where, depth, length), T, count = self._recorded(result, ('actions', 'rewards', 'where'))
        held = [actions, rewards, where, depth, length]
        boot = None
        if bootstrap is not None:
            b = bootstrap if isinstance(bootstrap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bootstrap, np.int32))
            b = b.to(self._dev).to(torch.int32).contiguous().reshape(-1)
            if int(b.numel()) != count:
                raise ValueError("bootstrap: int32 [%d] expected, got %d entries" % (count, int(b.numel())))
            held.append(b)
            boot = C.c_void_p(b.data_ptr())
        p = [C.c_void_p(x.data_ptr()) for x in (actions, rewards, where, depth, length)]
        h, L = self.env._h, _cabi.lib()
        use = int(self._grown is result)
        self._enqueue(lambda: L.ngw_tree_backup(h, t, *p, count, count, T, use, boot), held)

    def reweight(self, buckets=None):
        """Step 5: the rows of `buckets` recomputed from visits, returns, mask_words and priors.  buckets: None - every bucket the last backup
        (or iteration) touched -, or int32 bucket numbers (a list / numpy array or a device tensor; -1 is skipped).  Enqueued; no host wait."""
        import torch
        t = self._open()
        h, L = self.env._h, _cabi.lib()
        if buckets is None:
            self._enqueue(lambda: L.ngw_tree_reweight(h, t, None, 0))
            return
        b = buckets if isinstance(buckets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(buckets, np.int32))
        b = b.to(self._dev).to(torch.int32).contiguous().reshape(-1)
        n = int(b.numel())
        if n:
            self._enqueue(lambda: L.ngw_tree_reweight(h, t, C.c_void_p(b.data_ptr()), n), [b])

    # ------------------------------------------------------------------ reading
    def _where(self, keys_or_slots):
        """keys (numpy uint64 / torch int64) or pool slots (anything else) -> the buckets, a device tensor int32 [count]."""
        import torch
        x = keys_or_slots
        is_keys = (isinstance(x, torch.Tensor) and x.dtype == torch.int64) or (isinstance(x, np.ndarray) and x.dtype == np.uint64)
        if not is_keys:
            x = self.snap.keys(x, self.fields, device=True)
        return self.table.lookup(x, device=True)

    def read(self, keys_or_slots, device=False):
        """The statistics of states: TreeStats(where int32 [count] - the bucket, -1 where the table does not hold the state -, n int32
        [count, A] = visits, w int64 [count, A] = returns, mask uint64 [count]; zeros where `where` is -1).  keys_or_slots: state keys
        (numpy uint64, or a torch int64 tensor over the same bits) or slots of the pool (anything else that keys() takes).  A lookup and a
        gather; device=True: torch tensors (mask int64), no host wait - otherwise numpy arrays after one."""
        self._open()
        where = self._where(keys_or_slots)
        at = where.clamp(min=0).long()
        hit = where >= 0
        n = self.visits[at] * hit[:, None]
        w = self.returns[at] * hit[:, None]
        m = self.mask_words[at] * hit
        if device:
            return TreeStats(where, n, w, m)
        return TreeStats(where.cpu().numpy(), n.cpu().numpy(), w.cpu().numpy(), m.cpu().numpy().view(np.uint64))

    def best_actions(self, slots, device=False):
        """The most-visited VALID action of each state (keys or pool slots, as read() takes them): int32 [count], the lowest id on ties, -1
        where the state is not in the tree or its mask word was never learned.  What a caller commits after a search."""
        import torch
        self._open()
        where = self._where(slots)
        at = where.clamp(min=0).long()
        m = self.mask_words[at]
        valid = ((m[:, None] >> torch.arange(self.n_actions, device=self._dev)) & 1).bool() & (where >= 0)[:, None]
        n = torch.where(valid, self.visits[at].long(), torch.full((), -1, dtype=torch.int64, device=self._dev))
        best = n.max(dim=1, keepdim=True).values
        first = ((n == best) & valid).int().argmax(dim=1).int()                      # (argmax of a 0 / 1 tensor: the first 1)
        out = torch.where(valid.any(dim=1), first, torch.full_like(first, -1))
        return out if device else out.cpu().numpy()

    def stats(self):
        """TreeReport: iterations run since creation or clear(); alive / grown / refused / backed_up / depth, uint32 arrays with one entry per
        iteration of the last 64, oldest first - the pairs that executed a step, the nodes added, the leaves a full table refused, the steps
        backed up and the largest depth -; flags: the env's sticky flags (error_flags()), left standing.  Waits for the env's stream."""
        rep = _cabi.TreeReport()
        _cabi.check(_cabi.lib().ngw_tree_report(self.env._h, self._open(), C.byref(rep)))
        rows = np.ctypeslib.as_array(rep.stats).reshape(STATS_ROWS, 5)[:rep.rows].copy()
        return TreeReport(int(rep.iterations), *(rows[:, i] for i in range(5)), int(rep.flags))

    def clear(self):
        """Empties the TABLE and the statistics: visits, returns, mask words, rows and the report are zero, the iteration count is 0 and there
        are no roots (call start() again).  priors are the caller's and stay.  table.clear() alone does NOT clear the statistics."""
        t = self._open()
        h, L = self.env._h, _cabi.lib()
        self._grown = None
        self._enqueue(lambda: L.ngw_tree_clear(h, t))

    @property
    def closed(self):
        return not self._t

    def close(self):
        if self._t and self.env._h:
            _cabi.check(_cabi.lib().ngw_tree_destroy(self.env._h, self._t))
        self._invalidate()
        held = self.snap.__dict__.get('_searches')
        if held and self in held:
            held.remove(self)
        if self.__dict__.pop('owns_snapshot', False) and not self.snap.closed:
            self.snap.close()

    def _invalidate(self):
        """The handle is gone (or going), and the arrays with it."""
        self._t = C.c_void_p()
        self.visits = self.returns = self.mask_words = self.rows = self.priors = self.roots = self.where_leaf = self.last = None
        self._keep = self._grown = None
