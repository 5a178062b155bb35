"""The playout choice rule on the host: the public contract of include/ngw.h (ngw_snapshot_playout) in numpy, with a Philox4x32-10 of its
own - the counterpart of state_keys.keys_of_rows.  A host that knows a pair's state before step t (its valid-action mask word: env.action_mask_words,
Snapshot.action_masks) computes here the action the device drew for it:

    m = the mask word; all n_actions bits where it is 0
    w = word (t & 3) of Philox4x32-10, counter (t >> 2, 0, lo32(p), hi32(p)), key (lo32(seed), hi32(seed) ^ PLAYOUT_TAG)
    k = (w * popcount(m)) >> 32;  the action is the id of the (k + 1)-th set bit of m, counted from bit 0

p is the pair's global number (first_pair + its position in the call).  Nothing here touches the device."""
import collections

import numpy as np

PLAYOUT_TAG = 0x504C4159          # include/ngw.h NGW_PLAYOUT_TAG
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


class Playout(collections.namedtuple('Playout', 'ret length ended info first_action actions')):
    """What playout() / playouts() return: PlanEval's 'ret' int32, 'length' int32, 'ended' bool and 'info' uint32 (the last executed step's
    word), 'first_action' int32 (the action drawn at step 0: what a flat Monte-Carlo search groups the returns by), each [count] ([N, P] from
    playouts(), [P] on the single-env adapter), and 'actions' int32 [T, count] ([T, N, P]; [T, P]): the action of every executed step, -1 for
    a step the pair did not execute - or None where the call did not record them.  A named tuple whose fields can also be read by name:
    p['ret'].  numpy arrays, or torch tensors ('info' is int32 there, the same bits)."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    @property
    def goal(self):
        """The playout ended by the step itself reporting done (info bit 1, as on PlanEval; clear for a horizon cut)."""
        return self.ended & (((self.info >> 1) & 1) != 0)

    @property
    def died(self):
        """The playout ended in a FireWall death (message code 14)."""
        return self.ended & (((self.info >> 8) & 255) == 14)

    def shaped(self, *shape):
        """The per-pair fields reshaped to `shape`, the recorded actions to [T, *shape]."""
        a = self.actions
        return Playout(*[x.reshape(*shape) for x in self[:5]], None if a is None else a.reshape(a.shape[0], *shape))

    def row(self, i):
        """Env i's rows of an [N, P] result (the single-env adapter's view)."""
        a = self.actions
        return Playout(*[x[i] for x in self[:5]], None if a is None else a[:, i])


class PlayoutPath(collections.namedtuple('PlayoutPath', 'ret length ended info first_action actions keys')):
    """What playout(path_keys=True) / playouts(path_keys=True) return: Playout's fields and 'keys' [T, count] ([T, N, P]; [T, P]): entry
    (t, j) the key (state_keys) of the state pair j is in after it has executed step t, 0 for a step it did not execute - numpy uint64, or a
    torch int64 tensor over the same bits.  Flattened it is what KeyTable.insert takes, and snapshot.fresh_steps maps `fresh` back."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    goal = Playout.goal
    died = Playout.died

    def shaped(self, *shape):
        """The per-pair fields reshaped to `shape`, the recorded actions and the keys to [T, *shape]."""
        a, k = self.actions, self.keys
        return PlayoutPath(*[x.reshape(*shape) for x in self[:5]], None if a is None else a.reshape(a.shape[0], *shape), k.reshape(k.shape[0], *shape))

    def row(self, i):
        """Env i's rows of an [N, P] result (the single-env adapter's view)."""
        a = self.actions
        return PlayoutPath(*[x[i] for x in self[:5]], None if a is None else a[:, i], self.keys[:, i])


def pairs_symbol(kind, weighted=False, path=False, traj=False, views=False, guided=False):
    """The C entry point (include/ngw.h) behind one rollout / playout call: kind 'rollout' or 'playout'; traj - rewards, masks or observations are
    asked for; path - step limits or path keys are; weighted - a playout draws by weights; views - the observations are AgentMap views (a trajectory
    call by itself).  The form is the entry point's: views are `_traj_views`, any other traj is `_traj`, any other path `_path`, else the plain call
    (a weighted playout: `_weighted`; a rollout draws nothing).  guided - a playout looks its states up in a key table: `_playout_guided`, whatever
    else is set (a rollout takes plans: ValueError).  The one place that names the ten."""
    if kind not in ('rollout', 'playout'):
        raise ValueError("kind: 'rollout' or 'playout' expected, got %r" % (kind,))
    if guided:
        if kind != 'playout':
            raise ValueError("guided: a rollout takes plans, only a playout is guided by a key table")
        return 'ngw_snapshot_playout_guided'
    form = '_traj_views' if views else ('_traj' if traj else ('_path' if path else ('_weighted' if weighted and kind == 'playout' else '')))
    return 'ngw_snapshot_%s%s' % (kind, form)


OUTSIDE = {'default': 0, 'stop': 1}          # include/ngw.h NGW_OUTSIDE_*


def forward_keywords(path_keys=False, fields=None, rewards=False, masks=False, observe=None, view_size=5, table=None, table_weights=None, outside='default'):
    """The path, trajectory and guidance keywords a forwarding playouts() passes on: only those that are switched on (`fields` with path_keys or a
    table; `view_size` with observe='agent_view', or where it is not its default - the env then refuses it; `table_weights` and `outside` with a
    table, or where they are not their defaults - likewise), so a call without them is the call it always was."""
    kw = dict(path_keys=True, fields=fields) if path_keys else {}
    if table is not None:
        kw.update(table=table, fields=fields)
    if table_weights is not None:
        kw['table_weights'] = table_weights
    if table is not None or not (isinstance(outside, str) and outside == 'default'):
        kw['outside'] = outside
    if rewards:
        kw['rewards'] = True
    if masks:
        kw['masks'] = True
    if observe is not None:
        kw['observe'] = observe
    if observe == 'agent_view' or not (isinstance(view_size, int) and view_size == 5):
        kw['view_size'] = view_size
    return kw


def map_obs(obs, fn):
    """fn applied to the observation rows of a trajectory result: one array, the (beams, inventory) pair of the packed lidar format, or the dict
    of observe='agent_view' (fn on every value); None stays None."""
    if obs is None:
        return None
    if isinstance(obs, dict):
        return {k: fn(x) for k, x in obs.items()}
    return tuple(fn(x) for x in obs) if isinstance(obs, tuple) else fn(obs)


class PlayoutTraj(collections.namedtuple('PlayoutTraj', 'ret length ended info first_action actions keys rewards masks obs')):
    """What playout() / playouts() return with rewards=True, masks=True or observe='lidar': PlayoutPath's fields ('keys' None without
    path_keys) and, each None where it was not asked for,
      'rewards' int32 [T, count] ([T, N, P]; [T, P]): the reward of step t of pair j, 0 for a step it did not execute - rewards.sum(0) == ret;
      'masks'   uint64 [T, count] (a torch int64 tensor over the same bits): the valid-action word the choice of step t was made under, after
                the "no action would succeed -> every action" replacement, 0 for a step not executed - choose_actions(masks[t], seed, pairs, t, A)
                is actions[t];
      'obs'     [T + 1, count, row] ([T + 1, N, P, row]; [T + 1, P, row]) in the env's lidar format, as Snapshot.lidar_observation returns rows
                (the packed format: the pair (beams uint8, inventory int16)): obs[0] the parents, obs[t + 1] the state step t leaves (before any
                reset), all-zero rows for steps not executed.  (obs[t], actions[t], rewards[t], obs[t + 1]) is a transition for t < length;
                snapshot.transitions(result) lists those (t, j).  With observe='agent_view' it is the dict Snapshot.agent_view returns, every
                value with the same two leading axes: 'agent_map' int8 [T + 1, count, W, W], 'agent_facing_id' int32 [T + 1, count],
                'inventory_items_quantity' int32 [T + 1, count, K]."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    goal = Playout.goal
    died = Playout.died

    def shaped(self, *shape):
        """The per-pair fields reshaped to `shape`, the per-step fields to [T, *shape], the rows to [T + 1, *shape, row] (every value of a dict
        of views likewise: [T + 1, *shape, ...])."""
        def steps(x):
            return None if x is None else x.reshape(x.shape[0], *shape)
        return PlayoutTraj(*[x.reshape(*shape) for x in self[:5]], steps(self.actions), steps(self.keys), steps(self.rewards), steps(self.masks),
                           map_obs(self.obs, lambda x: x.reshape(x.shape[0], *shape, *x.shape[2:])))

    def row(self, i):
        """Env i's rows of an [N, P] result (the single-env adapter's view)."""
        def steps(x):
            return None if x is None else x[:, i]
        return PlayoutTraj(*[x[i] for x in self[:5]], steps(self.actions), steps(self.keys), steps(self.rewards), steps(self.masks), map_obs(self.obs, steps))


class PlayoutGuided(collections.namedtuple('PlayoutGuided', 'ret length ended info first_action actions keys rewards masks obs where depth')):
    """What playout() / playouts() return with table=: PlayoutTraj's fields (each per-step one None where it was not asked for) and
      'where' int32 [T, count] ([T, N, P]; [T, P]): the bucket KeyTable.lookup returns for the state pair j was in BEFORE step t, for every executed
              step; -1 where the table did not hold that state and -1 for a step the pair did not execute ('actions' tells the two apart);
      'depth' int32 [count] ([N, P]; [P]): the number of leading executed steps with where >= 0 - how far the pair stayed inside the table.
    tree_steps(result) lists the (bucket, action, t, j) of every executed in-table step: what a backup index_add_s into its [buckets, A] arrays."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    goal = Playout.goal
    died = Playout.died

    def shaped(self, *shape):
        """The per-pair fields reshaped to `shape`, the per-step fields to [T, *shape], the rows to [T + 1, *shape, row]."""
        t = PlayoutTraj(*self[:10]).shaped(*shape)
        return PlayoutGuided(*t, self.where.reshape(self.where.shape[0], *shape), self.depth.reshape(*shape))

    def row(self, i):
        """Env i's rows of an [N, P] result (the single-env adapter's view)."""
        return PlayoutGuided(*PlayoutTraj(*self[:10]).row(i), self.where[:, i], self.depth[i])


def tree_steps(result):
    """The executed in-table steps of a guided playout recorded with record=True: (bucket, action, t, j), four one-dimensional arrays of equal
    length - every (t, j) with result.where[t, j] >= 0, in step-major order; j indexes the flattened pair axes.  numpy int64 from a host result, torch
    int64 on the result's device otherwise (no host wait).  With them a backup over [buckets, A] tensors is one index_add_ each:
    N.view(-1).index_add_(0, bucket * A + action, ones) and Q.view(-1).index_add_(0, bucket * A + action, result.ret.reshape(-1)[j].float())."""
    where, actions = result.where, result.actions
    if actions is None:
        raise ValueError("tree_steps: the result holds no actions (playout(..., record=True) records them)")
    steps = int(where.shape[0])
    if hasattr(where, 'data_ptr'):
        import torch
        w, a = where.reshape(steps, -1), actions.reshape(steps, -1)
        n = max(int(w.shape[1]), 1)
        pos = torch.nonzero(w.reshape(-1) >= 0).reshape(-1)
        return w.reshape(-1)[pos].long(), a.reshape(-1)[pos].long(), torch.div(pos, n, rounding_mode='floor'), pos % n
    w, a = np.asarray(where).reshape(steps, -1), np.asarray(actions).reshape(steps, -1)
    pos = np.flatnonzero(w.reshape(-1) >= 0)
    t, j = divmod(pos, max(int(w.shape[1]), 1))
    return w.reshape(-1)[pos].astype(np.int64), a.reshape(-1)[pos].astype(np.int64), t, j


def check_guide(env, table, table_weights, outside, fields):
    """The guidance keywords of a playout, checked before a handle is touched -> None without a table, else (the outside flag, the fields word).
    table: a KeyTable of `env`, open; table_weights: required with it (its form is check_table_weights'); outside: 'default' or 'stop'; fields: a
    non-empty selection - it names the state that is looked up."""
    if not (isinstance(outside, str) and outside in OUTSIDE):
        raise ValueError("outside: 'default' or 'stop' expected, got %r" % (outside,))
    if table is None:
        if table_weights is not None:
            raise ValueError("table_weights without table: the rows belong to a key table's buckets")
        if outside != 'default':
            raise ValueError("outside=%r without table: there is no table to be outside of" % (outside,))
        return None
    from .key_table import KeyTable
    from .state_keys import KEY_STATE, check_fields
    if not isinstance(table, KeyTable):
        raise ValueError("table: a KeyTable expected")
    table._open_for(env)
    if table_weights is None:
        raise ValueError("table without table_weights: a float32 [table.buckets, A] array of weight rows expected")
    if fields is not None and not isinstance(fields, bool) and isinstance(fields, (int, np.integer)) and int(fields) == 0:
        raise ValueError("fields == 0: the look-up needs a non-empty selection of KEY_* bits")
    return OUTSIDE[outside], check_fields(KEY_STATE if fields is None else fields)


def check_table_weights(table_weights, buckets, n_actions, dev):
    """table_weights of a guided playout -> (a contiguous float32 torch tensor [buckets, n_actions] on `dev`, whether it was uploaded here).  A torch
    tensor must be exactly that and is used in place; anything else is a host array of that shape and is uploaded."""
    import torch
    shape = (int(buckets), int(n_actions))
    if isinstance(table_weights, torch.Tensor):
        if table_weights.dtype != torch.float32 or tuple(table_weights.shape) != shape or not table_weights.is_contiguous() or table_weights.device != dev:
            raise ValueError("table_weights: a contiguous float32 tensor %s on %s expected, got %s %s on %s" % (
                list(shape), dev, table_weights.dtype, list(table_weights.shape), table_weights.device))
        return table_weights, False
    w = np.asarray(table_weights)
    if w.dtype.kind not in 'fiu' or w.shape != shape:
        raise ValueError("table_weights: a float32 array %s expected, got %s %s" % (list(shape), w.dtype, list(w.shape)))
    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev), True


def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays: counter = four uint32 arrays (broadcastable), key = two -> the four output words, uint32 arrays."""
    c0, c1, c2, c3 = [np.asarray(x, np.uint64) & _LO for x in np.broadcast_arrays(*counter)]
    k0, k1 = [np.asarray(x, np.uint64) & _LO for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def playout_words(seed, pairs, t):
    """w of the contract for the global pair numbers `pairs` (uint64 values, any shape) at step t (an int, or an array broadcastable
    against pairs) -> uint32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p = np.asarray(pairs).astype(np.uint64)
    t = np.asarray(t, np.int64)
    if (t < 0).any():
        raise ValueError("t: steps are numbered from 0")
    p, t = np.broadcast_arrays(p, t)
    zero = np.zeros(p.shape, np.uint64)
    words = philox4x32_10(((t >> 2).astype(np.uint64), zero, p & _LO, p >> _S32), (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) ^ PLAYOUT_TAG)))
    return np.choose(t & 3, words)


def kth_set_bit(words, k):
    """The id of the (k + 1)-th set bit of each uint64 word, counted from bit 0 (k < popcount(word))."""
    w = np.asarray(words, np.uint64)
    bits = ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)
    return np.argmax(np.cumsum(bits, -1) > np.asarray(k, np.int64)[..., None], -1).astype(np.int32)


def choose_actions(mask_words, seed, pairs, t, n_actions):
    """The action the playout contract draws for each pair: mask_words = the uint64 valid-action words of the pairs' states before step t
    (int64 words over the same bits are taken too), pairs = their global pair numbers, t = the step (an int or an array), n_actions = the
    length of the action list.  -> int32, shaped as mask_words."""
    n_actions = int(n_actions)
    if not 1 <= n_actions < 64:
        raise ValueError("n_actions: %d outside [1, 64)" % n_actions)
    m = np.asarray(mask_words)
    m = m.view(np.uint64) if m.dtype == np.int64 else m.astype(np.uint64)
    every = np.uint64((1 << n_actions) - 1)
    if (m & ~every).any():
        raise ValueError("mask_words: a bit at or above n_actions = %d is set" % n_actions)
    m = np.where(m == 0, every, m)
    n = ((m[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).sum(-1).astype(np.uint64)
    w = np.broadcast_to(playout_words(seed, pairs, t), m.shape).astype(np.uint64)
    return kth_set_bit(m, (w * n) >> _S32)
