"""The model of the device-side key table (include/ngw.h ngw_key_table_*): a Python dict from key to first-seen order.  `fresh` is compared
exactly against it; `where` has no model - which bucket a key gets is not part of the contract - and is checked by its properties only:
equal <=> equal key, stable across calls, in range, -1 exactly where the model says.  Nothing here comes from the HIP path."""
import numpy as np


class KeyTableModel:
    """The keys ever inserted, in first-seen order.  Key 0 is never stored.  `buckets`: a table of that many buckets refuses a new key once
    it holds that many (None: never full)."""

    def __init__(self, buckets=None):
        self.order, self.buckets = {}, buckets

    def __len__(self):
        return len(self.order)

    def insert(self, keys):
        """-> (fresh bool [count], stored bool [count]): fresh[j] - keys[j] is new and j is its smallest position in this call; stored[j] -
        the table holds keys[j] after the call (False: key 0; without a bucket limit every other key is stored)."""
        keys = as_u64(keys).tolist()
        fresh, stored = np.zeros(len(keys), bool), np.zeros(len(keys), bool)
        for j, k in enumerate(keys):
            if k == 0:
                continue
            if k not in self.order:
                assert self.buckets is None or len(self.order) < self.buckets, "the model does not choose which keys a full table refuses"
                self.order[k] = len(self.order)
                fresh[j] = True
            stored[j] = True
        return fresh, stored

    def contains(self, keys):
        return np.array([k in self.order for k in as_u64(keys).tolist()], bool)


def as_u64(keys):
    """Keys as numpy uint64, whichever way they came back (numpy int64 / uint64, a torch int64 tensor)."""
    if hasattr(keys, 'data_ptr'):
        keys = keys.cpu().numpy()
    return np.ascontiguousarray(keys).astype(np.int64 if np.asarray(keys).dtype.kind == 'i' else np.uint64).view(np.uint64)


class WhereBook:
    """The properties of `where` across the calls of one table: every key keeps the bucket it was first reported in, no two keys share one,
    every bucket lies in [0, buckets), and -1 appears exactly where the key is not stored."""

    def __init__(self, buckets):
        self.buckets, self.of_key, self.of_bucket = int(buckets), {}, {}

    def check(self, keys, where, stored, what):
        keys, where = as_u64(keys).tolist(), np.asarray(where.cpu().numpy() if hasattr(where, 'data_ptr') else where)
        assert where.dtype == np.int32 and where.shape == (len(keys),), (what, where.dtype, where.shape)
        for j, (k, w, s) in enumerate(zip(keys, where.tolist(), np.asarray(stored).tolist())):
            if not s:
                assert w == -1, "%s: position %d, key %#x is not stored but where = %d" % (what, j, k, w)
                continue
            assert 0 <= w < self.buckets, "%s: position %d, where = %d outside [0, %d)" % (what, j, w, self.buckets)
            assert self.of_key.setdefault(k, w) == w, "%s: position %d, key %#x moved from bucket %d to %d" % (what, j, k, self.of_key[k], w)
            assert self.of_bucket.setdefault(w, k) == k, "%s: position %d, bucket %d holds %#x and %#x" % (what, j, w, self.of_bucket[w], k)

    def clear(self):
        self.of_key, self.of_bucket = {}, {}


class StandInEnv:
    """What a KeyTable or a Snapshot needs of its env before anything reaches the device: a handle that looks open and a device index."""
    _h, device, num_envs, n_actions = True, 0, 4, 5


def stand_in_table(capacity=8, env=None):
    """A KeyTable that looks open without a library call behind it: its host-side checks run, and raise, before anything would launch."""
    from gym_novel_gridworlds_amd.key_table import KeyTable, buckets_for
    t = KeyTable.__new__(KeyTable)
    t.env, t.capacity, t.buckets = env or StandInEnv(), int(capacity), buckets_for(capacity)
    t._t, t._keep = True, None
    return t


def stand_in_snapshot(capacity=8, env=None):
    """Likewise a Snapshot (Snapshot.copy's list checks)."""
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    s = Snapshot.__new__(Snapshot)
    s.env, s.capacity, s._s, s._keep = env or StandInEnv(), int(capacity), True, None
    return s
