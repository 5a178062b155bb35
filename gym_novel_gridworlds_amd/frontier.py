"""Device-side frontiers of a Snapshot: the step `flags -> the index lists of the next call` of a search loop without a host round trip
(include/ngw.h ngw_frontier_compact / ngw_frontier_alloc, NGW_IDX_NONE; the kernels are csrc/ngw_frontier.inc).

    fr = pool.frontier(capacity)                          # lists of `capacity` entries on the device, a slot cursor
    fr.reset_cursor(n_roots)                              # the next free slot of the pool
    for it in range(depth):                               # nothing in this loop waits for the host
        succ, found = pool.insert_successor_keys(table, parents, device=True)
        p, a = fr.fresh_pairs(found.fresh, parents)       # parent slot and action of every fresh child, padded with IDX_NONE
        c = fr.alloc()                                    # consecutive free slots for them, IDX_NONE where the pool is full
        pool.expand(p, a, c, device=True)                 # launched at `capacity`: a pair with an IDX_NONE index is skipped
        parents = c                                       # ... and so is it in the next iteration's keys and inserts
    fr.count(), fr.total()                                # the only host waits, and only when called

The same loop going on with the best k only (Frontier.select, include/ngw.h ngw_frontier_select; the kernels are csrc/ngw_select.inc) - a best-first
iteration over one pool and a valued key table, g[slot] the cost of the path to a slot:

        succ = pool.successor_keys(parents, device=True); g_child, tags = ...  # [count, A]: the cost of every child (key_table.py's loop)
        found = table.insert_min(succ.keys.reshape(-1), g_child.reshape(-1), tags=tags.reshape(-1), device=True)
        sel = fr.select(g_child, keep=k, div=A, map=parents, flags=found.best) # the k cheapest improved children; ties: the smaller position
        c = fr.alloc()                                    # count_dev[0] = taken: slots for exactly those
        pool.expand(sel.first, sel.second, c, device=True); parents = c        # sel.bound[0]: the cut, to compare with the goal's value

and a beam search of B states per env, env e's beam in the fixed slots e * B .. e * B + B - 1 of two pools that take turns:

        values = g[beam][:, None] + step_cost_values(succ.info, scale)         # [n_envs * B, A], VALUE_NONE where the parent is skipped
        sel = fr.select(values, keep=B, div=A, map=beam, groups=n_envs)        # per env the B cheapest of its B * A children
        other.expand(sel.first, sel.second, beam_slots, device=True)           # entry e * B + i: a padded pair is skipped, its slot keeps its row

snapshot.fresh_pairs / fresh_steps / transitions and playout.tree_steps return DENSE lists, for which torch.nonzero has to tell the host how
many there are; their twins here return lists of the frontier's fixed capacity whose live entries come first, in the same row-major order.
A list longer than the hits is padded with IDX_NONE; more hits than `capacity` keep the first `capacity` and raise the sticky
F_FRONTIER_FULL (error_flags()), with total() still the true number.  The returned `first`, `second` and `slots` are the frontier's own
tensors: the next compact / select / alloc overwrites them."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .key_table import VALUE_NONE                # include/ngw.h NGW_VALUE_NONE: the key table's "no offer"; never a candidate of a selection
from .spec import F_FRONTIER_FULL, IDX_NONE      # noqa: F401

MAX_FLAGS = 1 << 24          # csrc/ngw_device.h NGW_FRONTIER_MAX_FLAGS: the longest flag array of one call
MAX_CAPACITY = (1 << 31) - 1
SELECT_WAVE_MAX = 1024       # csrc/ngw_device.h NGW_SELECT_WAVE_MAX: up to this many values per group one wavefront selects, above it the grid form

Selected = collections.namedtuple('Selected', 'first second taken bound')


def check_capacity(capacity):
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)):
        raise ValueError("capacity: an integer expected, got %r" % (capacity,))
    if not 0 <= capacity <= MAX_CAPACITY:
        raise ValueError("capacity: %d outside [0, 2^31 - 1]" % capacity)
    return int(capacity)


def check_div(div):
    if isinstance(div, bool) or not isinstance(div, (int, np.integer)):
        raise ValueError("div: an integer expected, got %r" % (div,))
    if div < 1:
        raise ValueError("div: at least 1 expected, got %d" % div)
    return int(div)


def check_flag_count(n):
    if n > MAX_FLAGS:
        raise ValueError("flags: %d flags in one call (at most 2^24)" % n)
    return int(n)


def check_map_len(n_map, n, div):
    need = -(-n // div)
    if n_map < need:
        raise ValueError("map: %d entries for %d rows of flags" % (n_map, need))


def compact_reference(flags, div=1, map=None, capacity=None):
    """The contract of ngw_frontier_compact in numpy -> (first int32 [capacity], second int32 [capacity], count int32 [2], full bool).
    flags: a bool / uint8 array of any shape, read flattened - any non-zero byte counts; map: None or an int32 array of at least
    ceil(n / div) entries; capacity: None = the number of hits.  The positions p of the hits in ascending order; entry k < taken =
    min(total, capacity) is (map[p // div] or p // div, p % div), the entries behind are IDX_NONE; count = (taken, total); full = total >
    capacity (F_FRONTIER_FULL)."""
    f = np.asarray(flags)
    if f.dtype not in (np.bool_, np.uint8):
        raise ValueError("flags: a bool or uint8 array expected, got dtype %s" % f.dtype)
    f = f.reshape(-1).view(np.uint8)
    n, div = check_flag_count(f.size), check_div(div)
    if map is not None:
        map = np.asarray(map)
        if map.dtype != np.int32 or map.ndim != 1:
            raise ValueError("map: a one-dimensional int32 array expected, got dtype %s, shape %s" % (map.dtype, map.shape))
        check_map_len(map.size, n, div)
    pos = np.flatnonzero(f)
    total = int(pos.size)
    capacity = total if capacity is None else check_capacity(capacity)
    taken = min(total, capacity)
    q, r = np.divmod(pos[:taken], div)
    first = np.full(capacity, IDX_NONE, np.int32)
    second = np.full(capacity, IDX_NONE, np.int32)
    first[:taken] = q if map is None else map[q]
    second[:taken] = r
    return first, second, np.array([taken, total], np.int32), total > capacity


def check_select(n, groups, keep, capacity):
    """-> (groups, keep, m) of a selection among n values in a list of `capacity` entries (capacity None: not checked)."""
    for name, x in (('groups', groups), ('keep', keep)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError("%s: an integer expected, got %r" % (name, x))
    if n > MAX_FLAGS:
        raise ValueError("values: %d values in one call (at most 2^24)" % n)
    if not 1 <= groups <= MAX_FLAGS or n % groups:
        raise ValueError("groups: %d values do not make %d equal groups" % (n, groups))
    if not 0 <= keep <= MAX_CAPACITY:
        raise ValueError("keep: %d outside [0, 2^31 - 1]" % keep)
    if capacity is not None and groups * keep > capacity:
        raise ValueError("keep: %d groups of %d entries do not fit the capacity %d" % (groups, keep, capacity))
    return int(groups), int(keep), n // int(groups)


def select_reference(values, keep, div=1, map=None, flags=None, groups=1, largest=False, capacity=None):
    """The contract of ngw_frontier_select in numpy -> (first int32 [capacity], second int32 [capacity], taken int32 [groups], bound int32
    [groups], count int32 [2]).  values: an int32 array of any shape, read flattened as `groups` groups of m values; a candidate is a position
    whose value is not VALUE_NONE and whose flag (flags: None or a bool / uint8 array of as many bytes) is not zero.  Per group the candidates
    in the order (value ascending - descending with `largest` -, position ascending), the first taken = min(candidates, keep) of them chosen;
    entry g * keep + i is (map[p // div] or p // div, p % div) of the group's i-th chosen position p in ASCENDING POSITION order, every other
    entry IDX_NONE; bound = the value of the last chosen candidate in selection order, VALUE_NONE where none is; count = (taken[0] if groups
    == 1 else groups * keep, the candidates of all groups).  capacity: None = groups * keep."""
    v = np.asarray(values)
    if v.dtype != np.int32:
        raise ValueError("values: an int32 array expected, got dtype %s" % v.dtype)
    v = v.reshape(-1)
    n, div = v.size, check_div(div)
    capacity = None if capacity is None else check_capacity(capacity)
    groups, keep, m = check_select(n, groups, keep, capacity)
    capacity = groups * keep if capacity is None else capacity
    candidate = v != VALUE_NONE
    if flags is not None:
        f = np.asarray(flags)
        if f.dtype not in (np.bool_, np.uint8) or f.size != n:
            raise ValueError("flags: a bool or uint8 array of %d entries expected, got dtype %s, %d entries" % (n, f.dtype, f.size))
        candidate &= f.reshape(-1).view(np.uint8) != 0
    if map is not None:
        map = np.asarray(map)
        if map.dtype != np.int32 or map.ndim != 1:
            raise ValueError("map: a one-dimensional int32 array expected, got dtype %s, shape %s" % (map.dtype, map.shape))
        check_map_len(map.size, n, div)
    first = np.full(capacity, IDX_NONE, np.int32)
    second = np.full(capacity, IDX_NONE, np.int32)
    taken = np.zeros(groups, np.int32)
    bound = np.full(groups, VALUE_NONE, np.int32)
    for g in range(groups):
        pos = g * m + np.flatnonzero(candidate[g * m:(g + 1) * m])
        val = v[pos].astype(np.int64)
        order = np.lexsort((pos, -val if largest else val))          # stable: by value, then by position
        chosen = pos[order[:keep]]
        taken[g] = chosen.size
        if chosen.size:
            bound[g] = v[chosen[-1]]
        q, r = np.divmod(np.sort(chosen), div)
        first[g * keep:g * keep + chosen.size] = q if map is None else map[q]
        second[g * keep:g * keep + chosen.size] = r
    count = np.array([taken[0] if groups == 1 else groups * keep, np.count_nonzero(candidate)], np.int32)
    return first, second, taken, bound, count


def alloc_reference(count, cursor, limit, capacity):
    """The contract of ngw_frontier_alloc in numpy -> (slots int32 [capacity], the cursor afterwards, full bool): m = max(min(count, limit -
    cursor), 0) slots cursor .. cursor + m - 1, IDX_NONE behind them; full = m < count (F_FRONTIER_FULL)."""
    capacity = check_capacity(capacity)
    if limit < 0:
        raise ValueError("limit: %d is negative" % limit)
    m = max(min(int(count), int(limit) - int(cursor)), 0)
    slots = np.full(capacity, IDX_NONE, np.int32)
    k = min(m, capacity)
    slots[:k] = int(cursor) + np.arange(k)
    return slots, int(cursor) + m, m < int(count)


def _result_steps(result):
    """T of a rollout / playout result, read off the first per-step field it holds (as snapshot.transitions does)."""
    for name in ('rewards', 'masks', 'keys', 'actions', 'obs'):
        x = getattr(result, name, None)
        if x is not None:
            x = x[0] if isinstance(x, tuple) else (next(iter(x.values())) if isinstance(x, dict) else x)
            return int(x.shape[0]) - (1 if name == 'obs' else 0)
    raise ValueError("transitions: the result holds no per-step field")


class Frontier:
    """Index lists of `capacity` entries and a slot cursor in the env's device memory, for one Snapshot (Snapshot.frontier).  It owns
    `first`, `second`, `slots` (int32 [capacity]), `count_dev` (int32 [2]: the entries of the last compaction, and its hits) and `cursor` (int32 [1]:
    the next slot alloc() hands out).  Every method but count() and total() is enqueued and returns at once.  Closed by close() and with its
    snapshot."""

    def __init__(self, snap, capacity):
        import torch
        self.snap, self.env, self.capacity = snap, snap.env, check_capacity(capacity)
        snap._open()
        dev = torch.device('cuda:%d' % self.env.device)
        self.first = torch.full((self.capacity,), IDX_NONE, dtype=torch.int32, device=dev)
        self.second = torch.full((self.capacity,), IDX_NONE, dtype=torch.int32, device=dev)
        self.slots = torch.full((self.capacity,), IDX_NONE, dtype=torch.int32, device=dev)
        self.count_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self._dev = dev
        self._keep = None

    def _open(self):
        if self.first is None:
            raise ValueError("frontier is closed")
        self.snap._open()

    def _enqueue(self, call):
        from .snapshot import enqueue_ordered
        enqueue_ordered(self.env, self, call, 1, [], True)

    def compact(self, flags, div=1, map=None):
        """(first, second): the hits of `flags` - a contiguous bool / uint8 tensor on the env's device of any shape, read flattened; any
        non-zero byte counts - in ascending order: entry k is (map[p // div] or p // div, p % div) of the k-th hit's position p, IDX_NONE
        behind the hits.  For a [rows, div] flag array `first` is the row - through `map`, an int32 tensor of at least `rows` entries, e.g. the
        parent slot of each row - and `second` the column.  More hits than `capacity`: the first `capacity` are kept, F_FRONTIER_FULL is raised.
        Two kernel launches; no host wait."""
        import torch
        self._open()
        if not isinstance(flags, torch.Tensor) or flags.dtype not in (torch.bool, torch.uint8) or not flags.is_contiguous() or flags.device != self._dev:
            raise ValueError("flags: a contiguous bool or uint8 tensor on %s expected" % self._dev)
        n, div = check_flag_count(int(flags.numel())), check_div(div)
        if map is not None:
            if not isinstance(map, torch.Tensor) or map.dtype != torch.int32 or map.dim() != 1 or not map.is_contiguous() or map.device != self._dev:
                raise ValueError("map: a contiguous one-dimensional int32 tensor on %s expected" % self._dev)
            check_map_len(int(map.numel()), n, div)
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda: L.ngw_frontier_compact(h, C.c_void_p(flags.data_ptr()) if n else None, n, div,
                                                     C.c_void_p(map.data_ptr()) if map is not None and n else None, self.capacity,
                                                     C.c_void_p(self.first.data_ptr()) if self.capacity else None,
                                                     C.c_void_p(self.second.data_ptr()) if self.capacity else None, C.c_void_p(self.count_dev.data_ptr())))
        return self.first, self.second

    def select(self, values, keep, div=1, map=None, flags=None, groups=1, largest=False):
        """Selected(first, second, taken, bound): the `keep` best candidates of each of `groups` equal groups of `values` - a contiguous int32
        tensor on the env's device of any shape, read flattened; a candidate is a position whose value is not VALUE_NONE and, with `flags` (a
        contiguous bool / uint8 tensor of as many entries), whose flag is not zero.  Best is smallest, or largest with largest=True; among equal
        values the smaller position wins, so the same input selects the same entries in every run.  Entry g * keep + i of `first` / `second`
        (the frontier's lists) is (map[p // div] or p // div, p % div) of group g's i-th chosen position p in ascending position order -
        not sorted by value -, every other entry IDX_NONE; taken [groups] is how many each group chose, bound [groups] the value of the last
        one chosen - the cut -, VALUE_NONE where none was (new int32 tensors).  count() afterwards: taken[0] with one group - alloc() serves
        exactly the chosen -, groups * keep with more: alloc() hands a slot to every entry of the spans; total(): the candidates.  No flag
        is raised for what lies beyond `keep`.  One kernel launch for groups of up to 1024 values, six behind a memset above; no host wait."""
        import torch
        self._open()
        if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_contiguous() or values.device != self._dev:
            raise ValueError("values: a contiguous int32 tensor on %s expected" % self._dev)
        n, div = int(values.numel()), check_div(div)
        groups, keep, _ = check_select(n, groups, keep, self.capacity)
        if flags is not None:
            if not isinstance(flags, torch.Tensor) or flags.dtype not in (torch.bool, torch.uint8) or not flags.is_contiguous() or flags.device != self._dev:
                raise ValueError("flags: a contiguous bool or uint8 tensor on %s expected" % self._dev)
            if int(flags.numel()) != n:
                raise ValueError("flags: %d flags for %d values" % (int(flags.numel()), n))
        if map is not None:
            if not isinstance(map, torch.Tensor) or map.dtype != torch.int32 or map.dim() != 1 or not map.is_contiguous() or map.device != self._dev:
                raise ValueError("map: a contiguous one-dimensional int32 tensor on %s expected" % self._dev)
            check_map_len(int(map.numel()), n, div)
        taken = torch.empty(groups, dtype=torch.int32, device=self._dev)
        bound = torch.empty(groups, dtype=torch.int32, device=self._dev)
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda: L.ngw_frontier_select(h, C.c_void_p(values.data_ptr()) if n else None, C.c_void_p(flags.data_ptr()) if flags is not None and n else None,
                                                    n, groups, div, C.c_void_p(map.data_ptr()) if map is not None and n else None, keep, 1 if largest else 0,
                                                    self.capacity, C.c_void_p(self.first.data_ptr()) if self.capacity else None,
                                                    C.c_void_p(self.second.data_ptr()) if self.capacity else None, C.c_void_p(taken.data_ptr()),
                                                    C.c_void_p(bound.data_ptr()), C.c_void_p(self.count_dev.data_ptr())))
        return Selected(self.first, self.second, taken, bound)

    def alloc(self, limit=None):
        """slots: cursor, cursor + 1, ... for the entries of the last compaction - as many as `limit` (one past the last slot that may be
        handed out; None: the snapshot's capacity) leaves -, IDX_NONE behind them; the cursor moves on by as many.  Fewer than the compaction
        asked for: F_FRONTIER_FULL is raised, and the pairs whose slot is IDX_NONE are skipped by the call that takes the list.  One kernel
        launch; no host wait."""
        self._open()
        limit = self.snap.capacity if limit is None else limit
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 0 <= limit <= MAX_CAPACITY:
            raise ValueError("limit: an integer in [0, 2^31 - 1] expected, got %r" % (limit,))
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda: L.ngw_frontier_alloc(h, C.c_void_p(self.count_dev.data_ptr()), C.c_void_p(self.cursor.data_ptr()), int(limit), self.capacity,
                                                   C.c_void_p(self.slots.data_ptr()) if self.capacity else None))
        return self.slots

    def reset_cursor(self, start=0):
        """The next slot alloc() hands out (on torch's current stream; no host wait)."""
        self._open()
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start <= MAX_CAPACITY:
            raise ValueError("start: an integer in [0, 2^31 - 1] expected, got %r" % (start,))
        self.cursor.fill_(int(start))

    def count(self):
        """The live entries of the last compaction (waits for the device)."""
        self._open()
        return int(self.count_dev[0].item())

    def total(self):
        """The hits of the last compaction, also beyond the capacity (waits for the device)."""
        self._open()
        return int(self.count_dev[1].item())

    # ------------------------------------------------------------------ the padded twins of the dense helpers
    def fresh_pairs(self, fresh, parents=None):
        """snapshot.fresh_pairs at fixed capacity: (parent, action) int32 [capacity] of every True of a [count, A] `fresh`
        (insert_successor_keys(device=True)) in row-major order, IDX_NONE behind them.  parents: None - `parent` is the row of `fresh` - or
        the int32 device list the successor keys were computed for - `parent` is then the slot itself, ready for expand()."""
        return self.compact(fresh, int(fresh.shape[1]), parents)

    def best_pairs(self, values, parents, keep, groups=1, flags=None, largest=False):
        """fresh_pairs for the best only: (parent, action) int32 [capacity] of the `keep` best entries of each of `groups` groups of a [count,
        A] int32 `values` (select() says what best is and where the entries lie), ready for expand().  parents: None - `parent` is the row of
        `values` - or the int32 device list the values were computed for."""
        sel = self.select(values, keep, int(values.shape[1]), parents, flags, groups, largest)
        return sel.first, sel.second

    def fresh_steps(self, fresh):
        """snapshot.fresh_steps at fixed capacity: (step t, pair j) int32 [capacity] of every True of a [T, count] `fresh`, row-major."""
        return self.compact(fresh, max(int(fresh.shape[1]), 1))

    def transitions(self, result):
        """snapshot.transitions at fixed capacity: (step t, pair j) int32 [capacity] of every step a rollout / playout result on the device
        executed (t < length[j]), row-major."""
        import torch
        length = result.length.reshape(1, -1)
        steps = _result_steps(result)
        ran = torch.arange(steps, device=length.device, dtype=length.dtype)[:, None] < length
        return self.compact(ran.contiguous(), max(int(length.shape[1]), 1))

    def tree_steps(self, result):
        """playout.tree_steps at fixed capacity: (bucket, action, t, j) int32 [capacity] of every executed in-table step of a guided playout
        recorded with record=True (result.where[t, j] >= 0), step-major, IDX_NONE behind them.  t and j are the frontier's lists, bucket and
        action new tensors."""
        import torch
        where, actions = result.where, result.actions
        if actions is None:
            raise ValueError("tree_steps: the result holds no actions (playout(..., record=True) records them)")
        steps = int(where.shape[0])
        w, a = where.reshape(steps, -1), actions.reshape(steps, -1)
        n = max(int(w.shape[1]), 1)
        t, j = self.compact((w >= 0).contiguous(), n)
        live = t != IDX_NONE
        pos = torch.where(live, t.long() * n + j.long(), torch.zeros_like(t, dtype=torch.int64))
        none = torch.full_like(t, IDX_NONE)
        if w.numel() == 0:
            return none, none.clone(), t, j
        return torch.where(live, w.reshape(-1)[pos], none), torch.where(live, a.reshape(-1)[pos].to(torch.int32), none), t, j

    @property
    def closed(self):
        return self.first is None

    def close(self):
        if self.first is not None and self.env._h:
            self.env.sync()                     # (a queued call may still be writing the lists)
        self.first = self.second = self.slots = self.count_dev = self.cursor = None
        self._keep = None
