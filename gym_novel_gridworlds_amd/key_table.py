"""A device-side key table of a VecNovelGridworld: an open-addressing hash set of 64-bit keys in the env's device memory, so that a search
can ask "have I seen this state BEFORE?" across its iterations without carrying a sorted history of its own (include/ngw.h
ngw_key_table_*; the kernels are csrc/ngw_table.inc).

    table = env.key_table(1 << 20)                 # room for 2^20 states
    keys, found = pool.insert_keys(table, children)    # found.fresh[j]: children[j] holds a state no earlier call - and no earlier position - offered
    visits = torch.zeros(table.buckets, ...)       # per-state data is the caller's: arrays of table.buckets entries indexed by found.where
    archive.copy(children[found.fresh], free_slots, source=pool)       # keep the new ones

The table stores keys and nothing else - unless it is made with values=True.  Such a table also keeps, per key, the SMALLEST int32 value ever
offered with it and an int32 tag stored by the offer that brought that value (include/ngw.h ngw_key_table_insert_min / _read / _trace):
"is this the best way I have found to this state?".  A label-correcting search (uniform-cost and A* orderings are the caller's choice of
which improved states to expand) with nothing in the loop that waits for the host - no .item(), no nonzero:

    table = env.key_table(1 << 20, values=True)
    fr = pool.frontier(capacity); fr.reset_cursor(n_roots)
    keys, found = pool.insert_keys_min(table, roots, torch.zeros(n_roots, ...), device=True)       # the roots: value 0, tag TAG_ROOT
    g = torch.full((pool.capacity,), VALUE_NONE, ...); g[roots] = 0                               # the cost each slot was reached with
    bucket = torch.full((pool.capacity,), -1, ...); bucket[roots] = found.where                   # ... and the bucket of its state
    for it in range(depth):
        succ = pool.successor_keys(parents, device=True)                                          # [P, A] keys and info words; parents: slots, IDX_NONE-padded
        live = (parents != IDX_NONE)[:, None]; pi = parents.clamp(min=0).long()
        g_child = torch.where(live, g[pi][:, None] + step_cost_values(succ.info), VALUE_NONE)     # (a skipped parent's keys are 0 anyway)
        tags = bucket[pi][:, None] * A + torch.arange(A, ...)                                     # parent_bucket * A + action: what trace() reads
        found = table.insert_min(succ.keys.reshape(-1), g_child.reshape(-1), tags=tags.reshape(-1), device=True)
        p, a = fr.compact(found.best, A, parents)                                                 # the (parent, action) of every state reached more cheaply
        c = fr.alloc()                                                                            # ... new OR seen before at a higher cost: reopened
        pool.expand(p, a, c, device=True)
        # g[c], bucket[c] = the children's values and buckets: gather g_child and found.where at p's rows (Frontier keeps the order of `best`)
        parents = c
    t = table.trace(table.lookup(goal_keys, device=True), steps, device=True)                     # the cheapest plan found to each goal, from its root
    pool.rollout(root_slot_of[t.root], t.plans, limits=t.length.clamp(0, steps), children=c, device=True)

The same loop as one object: s = pool.search(table, capacity); s.start(roots); s.run(depth) enqueues `depth` of these iterations from one
call, keeps g and bucket itself and records the cheapest goal reached (search.py; include/ngw.h ngw_search_*).  The loop above stays what an
iteration IS, and the form to write when a step of it has to differ.

All calls run on the env's stream, in the order they are made; concurrent inserts into one table from two streams are not supported."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .snapshot import enqueue_ordered, tensor_len, upload
from .spec import IDX_NONE, STEP_COSTS

VALUE_NONE = (1 << 31) - 1        # include/ngw.h NGW_VALUE_NONE: "never valued"; as an offered value: no offer
TAG_ROOT = -1                     # include/ngw.h NGW_TAG_ROOT: the tag of a bucket before any is stored; trace() ends a chain there
TRACE_MAX_STEPS = 1 << 16         # include/ngw.h NGW_TRACE_MAX_STEPS
MAX_MIN_COUNT = (1 << 31) - 1     # the keys of one insert_min / the queries of one trace


class KeyInsert(collections.namedtuple('KeyInsert', 'where fresh')):
    """What KeyTable.insert() returns: where int32 [count] (the bucket of each key, -1: key 0 or a full table), fresh bool [count]."""
    __slots__ = ()


class KeyBest(collections.namedtuple('KeyBest', 'where fresh best')):
    """What KeyTable.insert_min() returns: where and fresh as on KeyInsert, best bool [count] - this position brought its key a smaller value
    than the table held (at most one position per key and call)."""
    __slots__ = ()


class Trace(collections.namedtuple('Trace', 'plans length root')):
    """What KeyTable.trace() returns: plans int32 [steps, count] (column j: the actions from the root to bucket where[j] in execution
    order, -1 behind them), length int32 [count] (-1: no chain to a root within `steps` links), root int32 [count] (the bucket the chain
    ends in, -1 with length -1)."""
    __slots__ = ()


def buckets_for(capacity):
    """The buckets of a table of `capacity` keys: the smallest power of two >= 2 * capacity (a load of at most one half)."""
    capacity = int(capacity)
    if not 1 <= capacity <= 1 << 29:
        raise ValueError("capacity: %d outside [1, 2^29]" % capacity)
    return 1 << (2 * capacity - 1).bit_length()


def check_keys(keys, device_len=None):
    """The host-side check of one key list: a list / numpy array of one dimension and integer dtype -> a contiguous int64 array over the same
    64 bits (uint64 keys above 2^63 wrap to negative numbers: the bits are the key); device_len(x): the length of x when it is a device
    tensor to be used in place, else None.  Returns (keys, count)."""
    n = None if device_len is None else device_len(keys)
    if n is not None:
        return keys, int(n)
    if keys is None:
        raise ValueError("keys: a list of 64-bit keys expected")
    a = np.asarray(keys)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int64), 0          # (an empty list has no dtype of its own)
    if a.dtype.kind not in 'iu':
        raise ValueError("keys: integer keys expected, got dtype %s" % a.dtype)
    if a.ndim != 1:
        raise ValueError("keys: a one-dimensional key list expected, got shape %s" % (a.shape,))
    a = a.astype(np.uint64 if a.dtype.kind == 'u' else np.int64)
    return np.ascontiguousarray(a).view(np.int64), int(a.size)


def check_i32(x, name, count=None, device_len=None):
    """The host-side check of one int32 list (values, tags, buckets): a list / numpy array of one dimension and integer dtype whose entries fit
    an int32 -> a contiguous int32 array; device_len(x): the length of x when it is a device tensor to be used in place, else None.  With
    `count`, the list must have that many entries.  Returns (list, its length)."""
    n = None if device_len is None else device_len(x)
    if n is None:
        if x is None:
            raise ValueError("%s: a list of int32 expected" % name)
        a = np.asarray(x)
        if a.size == 0 and a.ndim == 1:
            a = np.zeros(0, np.int32)
        if a.dtype.kind not in 'iu':
            raise ValueError("%s: integers expected, got dtype %s" % (name, a.dtype))
        if a.ndim != 1:
            raise ValueError("%s: a one-dimensional list expected, got shape %s" % (name, a.shape))
        if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) > (1 << 31) - 1):
            raise ValueError("%s: an entry does not fit an int32" % name)
        x, n = np.ascontiguousarray(a.astype(np.int32)), int(a.size)
    if count is not None and n != count:
        raise ValueError("%s: %d entries for %d keys" % (name, n, count))
    return x, int(n)


def step_cost_values(info_words, scale=1):
    """int32 values for insert_min from the packed info words successor_keys / expand / lookahead report (include/ngw.h NGW_INFO_*: the step
    cost's code in bits 2..7): round(STEP_COSTS[code] * scale), of the words' shape - a numpy array for a numpy array, a torch int32 tensor on
    the words' device for a torch tensor (no host wait).
    The arithmetic is the caller's: values are int32, VALUE_NONE = 2^31 - 1 means "no offer", and g + cost wraps silently beyond it.  The
    largest step cost is 50 000, so a path of L steps costs at most L * round(50 000 * scale): keep L * 50 000 * scale below 2^31 - 1 -
    42 949 steps at scale 1, 429 at scale 100 (two of the costs are not integers; scale = 1000000 keeps 27.906975 exact and leaves no room
    for the 50 000).  A scale under which a single cost reaches VALUE_NONE is refused here."""
    lut = [int(round(c * scale)) for c in STEP_COSTS]
    if not all(0 <= v < VALUE_NONE for v in lut):
        raise ValueError("scale: %r takes a step cost outside [0, 2^31 - 1)" % (scale,))
    lut += [0] * (64 - len(lut))
    if hasattr(info_words, 'data_ptr'):
        import torch
        table = torch.tensor(lut, dtype=torch.int32, device=info_words.device)
        return table[((info_words >> 2) & 63).long()]
    return np.asarray(lut, np.int32)[(np.asarray(info_words).astype(np.int64) >> 2) & 63]


def insert_min_reference(held, keys, values, tags=None, refused=None):
    """The contract of ngw_key_table_insert_min in plain Python -> (stored bool [count], fresh bool [count], best bool [count]).
    held: the table before the call, a dict key -> [value, tag] (VALUE_NONE / TAG_ROOT: never valued), updated in place to the table after
    it.  refused: None, or a bool array - positions a full table turned away (where = -1; the table's choice, not the contract's): they store
    nothing, are neither fresh nor best and make no offer.  Key 0 is never stored.
    fresh[j]: keys[j] was not held and j is its first stored position.  The offer for a key: the position with the smallest (values[j], j)
    among its stored positions whose value is not VALUE_NONE; best[j]: j is the offer and values[j] < the value held before the call."""
    keys = np.asarray(keys)
    keys = keys.astype(np.int64 if keys.dtype.kind == 'i' else np.uint64).view(np.uint64).tolist()
    values, _ = check_i32(values, 'values', len(keys))
    if tags is not None:
        tags, _ = check_i32(tags, 'tags', len(keys))
    n = len(keys)
    stored, fresh, best = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    offer = {}
    for j, k in enumerate(keys):
        if k == 0 or (refused is not None and refused[j]):
            continue
        stored[j] = True
        if k not in held:
            held[k] = [VALUE_NONE, TAG_ROOT]
            fresh[j] = True
        v = int(values[j])
        if v != VALUE_NONE and (k not in offer or v < int(values[offer[k]])):
            offer[k] = j                          # (ascending j: an equal value keeps the earlier position)
    for k, j in offer.items():
        if int(values[j]) < held[k][0]:
            best[j] = True
            held[k][0] = int(values[j])
            if tags is not None:
                held[k][1] = int(tags[j])
    return stored, fresh, best


def trace_reference(where, steps, n_actions, occupied, tags):
    """The contract of ngw_key_table_trace in plain Python -> (plans int32 [steps, count], length int32 [count], root int32 [count], bad bool:
    F_BAD_INDEX).  occupied: bool [buckets] - the bucket holds a key; tags: int [buckets]."""
    where = np.asarray(where).reshape(-1)
    buckets, A = len(occupied), int(n_actions)
    plans = np.full((steps, where.size), -1, np.int32)
    length, root, bad = np.full(where.size, -1, np.int32), np.full(where.size, -1, np.int32), False
    for j, w in enumerate(where.tolist()):
        if w in (-1, IDX_NONE):
            continue
        b, moves = w, []
        while True:
            if not 0 <= b < buckets or not occupied[b]:
                bad = True
                break
            tg = int(tags[b])
            if tg == TAG_ROOT:
                length[j], root[j] = len(moves), b
                plans[:len(moves), j] = moves[::-1]
                break
            if len(moves) == steps:
                break                             # (no root after `steps` links: not an error)
            if not 0 <= tg < buckets * A:
                bad = True
                break
            b, a = divmod(tg, A)
            moves.append(a)
    return plans, length, root, bad


class KeyTable:
    """An open-addressing hash set of 64-bit keys with room for `capacity` of them in `buckets` (the smallest power of two >= 2 * capacity)
    buckets; with values=True it also holds an int32 value and an int32 tag per key (insert_min / read / get / trace; a plain insert()
    leaves both alone).  Belongs to the env that made it (VecNovelGridworld.key_table); closed by close(), by the env's close() and by an in-place
    rebuild() (inject_novelty) - a closed table raises on use.

    keys: a list / numpy array of integers (checked on the host - one dimension, integer dtype - and uploaded), or a contiguous
    one-dimensional torch int64 tensor on the env's device, used in place: exactly what Snapshot.keys(device=True) returns.  The tensor must
    be complete on torch's current stream before the call and must not be changed until the env's stream has passed the call.
    Key 0 is never stored: it is the empty-bucket mark, and the key of a bad index (which has raised F_BAD_INDEX already)."""

    values = False                              # made with values=True: insert_min / read / get / trace

    def __init__(self, env, capacity, values=False, *, _first_sequence=0):
        self.env, self.capacity, self.buckets = env, int(capacity), buckets_for(capacity)
        self.values = bool(values)
        self._t = C.c_void_p()
        self._keep = None                       # an uploaded key list the last call may still be reading
        if self.values:                         # (_first_sequence: where the table's position counter starts - no result depends on it; a seam for tests)
            _cabi.check(_cabi.lib().ngw_key_table_create_valued(env._h, self.capacity, int(_first_sequence), C.byref(self._t)))
        elif _first_sequence:
            raise ValueError("_first_sequence: only a table with values has one")
        else:
            _cabi.check(_cabi.lib().ngw_key_table_create(env._h, self.capacity, C.byref(self._t)))

    def _open(self):
        if not self._t or not self.env._h:
            raise ValueError("key table is closed")
        return self._t

    def _open_for(self, env):
        self._open()
        if self.env is not env:
            raise ValueError("table: a key table of another env")

    def _keys_arg(self, keys):
        """`keys` of one call, checked and uploaded -> (device pointer or None, count, torch device, [the uploaded tensor] or [])."""
        import torch
        self._open()
        dev = torch.device('cuda:%d' % self.env.device)
        k, count = check_keys(keys, lambda x: tensor_len(dev, 'keys', x, 'int64'))
        (ptr,), uploaded = upload(dev, count, k)
        return ptr, count, dev, uploaded

    def insert(self, keys, device=False):
        """Offers `keys` to the table: KeyInsert(where, fresh), both [count].
        fresh[j] is True exactly when keys[j] was not in the table before this call AND j is the smallest position that holds that key in
        this call (the `first` convention of Snapshot.unique()).  It is deterministic: it does not depend on the order in which the device
        runs the keys.
        where[j] (int32) is the bucket that holds keys[j]: equal keys get equal `where`, in this call and in every later one until clear();
        different keys get different `where`; every value lies in [0, buckets).  WHICH bucket a key gets is not part of the contract - it may
        depend on races between different keys that collide -, so index per-state arrays of `buckets` entries with it and do not compare it
        between tables or runs.
        Key 0: where = -1, fresh = False, no flag.  A key that finds neither itself nor a free bucket after probing EVERY bucket is refused:
        where = -1, fresh = False, and the env's sticky F_TABLE_FULL is raised (error_flags()); there is no shorter probe limit, so a refusal
        means that the table really is full.
        device=True: torch tensors on the env's device (where int32, fresh bool), ordered behind the launches on torch's current stream - no
        copy, no host wait; otherwise numpy arrays after one sync.  Two kernel launches."""
        import torch
        env, t = self.env, self._open()
        ptr, count, dev, uploaded = self._keys_arg(keys)
        where = torch.empty(count, dtype=torch.int32, device=dev)
        fresh = torch.empty(count, dtype=torch.uint8, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_key_table_insert(env._h, t, ptr, count, C.c_void_p(where.data_ptr()),
                                                                            C.c_void_p(fresh.data_ptr())), count, uploaded, device)
        if device:
            return KeyInsert(where, fresh.view(torch.bool))
        return KeyInsert(where.cpu().numpy(), fresh.cpu().numpy().view(np.bool_))

    def lookup(self, keys, device=False):
        """where int32 [count]: the bucket that holds keys[j] - the value insert() reported for that key -, or -1 where the table does not
        hold it (key 0 included).  It changes nothing.  One kernel launch; keys and device as in insert()."""
        import torch
        env, t = self.env, self._open()
        ptr, count, dev, uploaded = self._keys_arg(keys)
        where = torch.empty(count, dtype=torch.int32, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_key_table_lookup(env._h, t, ptr, count, C.c_void_p(where.data_ptr())), count, uploaded,
                        device)
        return where if device else where.cpu().numpy()

    def _valued(self):
        self._open()
        if not self.values:
            raise ValueError("a key table without values: make it with key_table(capacity, values=True)")

    def _i32_args(self, count, **lists):
        """int32 lists of one call (None passes), each checked against `count` (None: the first list sets it) -> (checked lists, count, device)."""
        import torch
        dev = torch.device('cuda:%d' % self.env.device)
        out = []
        for name, x in lists.items():
            if x is not None:
                x, count = check_i32(x, name, count, lambda y, name=name: tensor_len(dev, name, y))
            out.append(x)
        return out, count, dev

    def insert_min(self, keys, values, tags=None, device=False):
        """insert() that also offers a value with every key: KeyBest(where, fresh, best), each [count].  where and fresh are exactly
        insert()'s for the same keys - an insert_min IS an insert: the same buckets, the same F_TABLE_FULL, the same treatment of key 0.
        best[j] is True exactly when j is its key's OFFER - the position with the smallest (values[j], j) among the positions of this call
        that carry the key, are stored (where >= 0) and whose value is not VALUE_NONE - and values[j] is SMALLER than the value the table
        held for the key before the call (VALUE_NONE where it was absent or never valued; an equal value of a later call is no improvement).
        Afterwards the table holds the smaller of the two, and where best[j] is True and tags were given, tags[j].  At most one position per
        key is best, and which one does not depend on the order the device runs them in, nor on the buckets.  A value of VALUE_NONE makes no
        offer (the position behaves as under insert()); every other int32 - negative, INT32_MIN - is an ordinary value.
        values, tags: lists / numpy arrays of `count` integers that fit an int32 (checked and uploaded), or contiguous one-dimensional torch
        int32 tensors on the env's device, used in place under the rules of `keys`.  At most 2^31 - 1 keys.  Two kernel launches."""
        import torch
        env, t = self.env, self._open()
        self._valued()
        k, count = check_keys(keys, lambda x: tensor_len(torch.device('cuda:%d' % env.device), 'keys', x, 'int64'))
        if count > MAX_MIN_COUNT:
            raise ValueError("keys: %d keys in one insert_min (at most 2^31 - 1)" % count)
        (v, g), count, dev = self._i32_args(count, values=values, tags=tags)
        if v is None:
            raise ValueError("values: a list of int32 expected")
        (kp, vp, gp), uploaded = upload(dev, count, k, v, g)
        where = torch.empty(count, dtype=torch.int32, device=dev)
        fresh = torch.empty(count, dtype=torch.uint8, device=dev)
        best = torch.empty(count, dtype=torch.uint8, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_key_table_insert_min(env._h, t, kp, vp, gp, count, C.c_void_p(where.data_ptr()),
                                                                                C.c_void_p(fresh.data_ptr()), C.c_void_p(best.data_ptr())),
                        count, uploaded, device)
        if device:
            return KeyBest(where, fresh.view(torch.bool), best.view(torch.bool))
        return KeyBest(where.cpu().numpy(), fresh.cpu().numpy().view(np.bool_), best.cpu().numpy().view(np.bool_))

    def read(self, where, device=False):
        """(value, tag), int32 [count]: what the table holds in the buckets `where` (what insert / insert_min / lookup reported; a list of
        integers, or a torch int32 tensor on the env's device, used in place).  -1 and IDX_NONE give (VALUE_NONE, TAG_ROOT); so does any
        other bucket outside [0, buckets), which also raises F_BAD_INDEX; so does a bucket whose key was never valued.  One kernel launch;
        it changes nothing.  device: as in insert()."""
        import torch
        env, t = self.env, self._open()
        self._valued()
        (w,), count, dev = self._i32_args(None, where=where)
        if w is None:
            raise ValueError("where: a list of buckets expected")
        (wp,), uploaded = upload(dev, count, w)
        value = torch.empty(count, dtype=torch.int32, device=dev)
        tag = torch.empty(count, dtype=torch.int32, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_key_table_read(env._h, t, wp, count, C.c_void_p(value.data_ptr()), C.c_void_p(tag.data_ptr())),
                        count, uploaded, device)
        return (value, tag) if device else (value.cpu().numpy(), tag.cpu().numpy())

    def get(self, keys, device=False):
        """(value, tag) of `keys`: lookup() followed by read(), the buckets left on the device in between - no host wait there.  A key the
        table does not hold gives (VALUE_NONE, TAG_ROOT)."""
        self._valued()
        return self.read(self.lookup(keys, device=True), device=device)

    def trace(self, where, steps, n_actions=None, device=False):
        """The way back from the buckets `where` to their roots, read from the tags under the convention tag = parent_bucket * n_actions +
        action (what the loop in this module's docstring stores; n_actions None: the env's): Trace(plans int32 [steps, count], length int32
        [count], root int32 [count]).  Column j of `plans` holds the actions from the root to bucket where[j] in execution order, -1 behind
        them - the step-major layout of walk_plans and playout(record=True).actions, so rollout(roots, plans, limits=length.clamp(0, steps),
        children=c) replays it with the tensors left on the device; root[j] is the bucket the chain ends in: the one whose tag is TAG_ROOT.
        At most `steps` links are followed, because tags are the caller's data and may form cycles: a chain with no root after `steps` links
        gives length -1, root -1 and a column of -1, without a flag; so does where[j] of -1 or IDX_NONE.  A bucket on the chain outside the
        table or without a key, or a tag outside [0, buckets * n_actions), gives the same and raises F_BAD_INDEX; no tag is used as an
        address unchecked.  buckets * n_actions must not exceed 2^31 - 1 (ValueError).  One kernel launch, one lane per query."""
        import torch
        env, t = self.env, self._open()
        self._valued()
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 0 <= steps <= TRACE_MAX_STEPS:
            raise ValueError("steps: an integer in [0, %d] expected, got %r" % (TRACE_MAX_STEPS, steps))
        A = env.n_actions if n_actions is None else n_actions
        if isinstance(A, bool) or not isinstance(A, (int, np.integer)) or A < 1:
            raise ValueError("n_actions: a positive integer expected, got %r" % (A,))
        if self.buckets * int(A) > (1 << 31) - 1:
            raise ValueError("trace: buckets * n_actions = %d does not fit a tag (at most 2^31 - 1)" % (self.buckets * int(A)))
        (w,), count, dev = self._i32_args(None, where=where)
        if w is None:
            raise ValueError("where: a list of buckets expected")
        if count > MAX_MIN_COUNT:
            raise ValueError("where: %d buckets in one trace (at most 2^31 - 1)" % count)
        (wp,), uploaded = upload(dev, count, w)
        steps, A = int(steps), int(A)
        plans = torch.empty((steps, count), dtype=torch.int32, device=dev)
        length = torch.empty(count, dtype=torch.int32, device=dev)
        root = torch.empty(count, dtype=torch.int32, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_key_table_trace(env._h, t, wp, count, steps, A, C.c_void_p(plans.data_ptr()) if steps else None,
                                                                           C.c_void_p(length.data_ptr()), C.c_void_p(root.data_ptr())),
                        count, uploaded, device)
        return Trace(plans, length, root) if device else Trace(plans.cpu().numpy(), length.cpu().numpy(), root.cpu().numpy())

    def __len__(self):
        """The number of keys in the table (waits for the env's stream)."""
        n = C.c_int64(0)
        _cabi.check(_cabi.lib().ngw_key_table_count(self.env._h, self._open(), C.byref(n)))
        return int(n.value)

    def clear(self):
        """Empties the table, values and tags included (on the env's stream; no host wait).  Buckets reported earlier mean nothing afterwards.
        It does NOT clear the statistics a TreeSearch keeps per bucket of this table (visits, returns, mask words, rows): TreeSearch.clear()
        clears both."""
        _cabi.check(_cabi.lib().ngw_key_table_clear(self.env._h, self._open()))

    @property
    def closed(self):
        return not self._t

    def close(self):
        if self._t and self.env._h:
            _cabi.check(_cabi.lib().ngw_key_table_destroy(self.env._h, self._t))
        self._invalidate()
        tables = self.env.__dict__.get('_key_tables')
        if tables and self in tables:
            tables.remove(self)

    def _invalidate(self):
        """The handle is gone (or going), and the buffer with it."""
        self._t = C.c_void_p()
        self._keep = None
