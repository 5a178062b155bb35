"""A device-side key table of a VecNovelGridworld: an open-addressing hash set of 64-bit keys in the env's device memory, so that a search
can ask "have I seen this state BEFORE?" across its iterations without carrying a sorted history of its own (include/ngw.h
ngw_key_table_*; the kernels are csrc/ngw_table.inc).

    table = env.key_table(1 << 20)                 # room for 2^20 states
    keys, found = pool.insert_keys(table, children)    # found.fresh[j]: children[j] holds a state no earlier call - and no earlier position - offered
    visits = torch.zeros(table.buckets, ...)       # per-state data is the caller's: arrays of table.buckets entries indexed by found.where
    archive.copy(children[found.fresh], free_slots, source=pool)       # keep the new ones

The table stores keys and nothing else.  All calls run on the env's stream, in the order they are made; concurrent inserts into one table
from two streams are not supported."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .snapshot import enqueue_ordered, tensor_len, upload


class KeyInsert(collections.namedtuple('KeyInsert', 'where fresh')):
    """What KeyTable.insert() returns: where int32 [count] (the bucket of each key, -1: key 0 or a full table), fresh bool [count]."""
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


class KeyTable:
    """An open-addressing hash set of 64-bit keys with room for `capacity` of them in `buckets` (the smallest power of two >= 2 * capacity)
    buckets.  Belongs to the env that made it (VecNovelGridworld.key_table); closed by close(), by the env's close() and by an in-place
    rebuild() (inject_novelty) - a closed table raises on use.

    keys: a list / numpy array of integers (checked on the host - one dimension, integer dtype - and uploaded), or a contiguous
    one-dimensional torch int64 tensor on the env's device, used in place: exactly what Snapshot.keys(device=True) returns.  The tensor must
    be complete on torch's current stream before the call and must not be changed until the env's stream has passed the call.
    Key 0 is never stored: it is the empty-bucket mark, and the key of a bad index (which has raised F_BAD_INDEX already)."""

    def __init__(self, env, capacity):
        self.env, self.capacity, self.buckets = env, int(capacity), buckets_for(capacity)
        self._t = C.c_void_p()
        self._keep = None                       # an uploaded key list the last call may still be reading
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

    def __len__(self):
        """The number of keys in the table (waits for the env's stream)."""
        n = C.c_int64(0)
        _cabi.check(_cabi.lib().ngw_key_table_count(self.env._h, self._open(), C.byref(n)))
        return int(n.value)

    def clear(self):
        """Empties the table (on the env's stream; no host wait).  Buckets reported earlier mean nothing afterwards."""
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
