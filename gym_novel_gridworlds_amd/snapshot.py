"""Device-side snapshots of a VecNovelGridworld: save, restore and fork env states by index without leaving the GPU
(include/ngw.h ngw_snapshot_*; the kernel is csrc/ngw_snapshot.inc).

    snap = env.snapshot()                      # one slot per env
    snap.save()                                # slot i := env i
    ...
    snap.restore()                             # env i := slot i: the envs are back where they were, episode counters included
    snap.restore(slots=best, envs=worst)       # population methods: the states saved from the best envs over the worst
    env.fork(src)                              # env e := env src[e]

What a restored env does next: env e, when it next resets, draws from env e's OWN stream at its (restored or kept) episode counter.  Two
forks of one slot share the rest of the current episode and differ from their next reset on; restoring the same env from the same slot
twice replays the same future.  reward / done / info of the last step are not part of a snapshot."""
import ctypes as C

import numpy as np

from . import _cabi

KEEP_EPISODE = 1          # include/ngw.h NGW_SNAP_KEEP_EPISODE


def check_indices(idx, limit, distinct=False, name='index'):
    """The host-side check of one index argument given as a list / numpy array: integer dtype, one dimension, every value in
    [0, limit), and no value twice where `distinct`.  Returns a contiguous int32 array (None stays None); ValueError otherwise."""
    if idx is None:
        return None
    a = np.asarray(idx)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int32)            # (an empty list has no dtype of its own)
    if a.dtype.kind not in 'iu':
        raise ValueError("%s: integer indices expected, got dtype %s" % (name, a.dtype))
    if a.ndim != 1:
        raise ValueError("%s: a one-dimensional index list expected, got shape %s" % (name, a.shape))
    if a.size:
        lo, hi = int(a.min()), int(a.max())
        if lo < 0 or hi >= limit:
            raise ValueError("%s: %d outside [0, %d)" % (name, lo if lo < 0 else hi, limit))
        if distinct and np.unique(a).size != a.size:
            raise ValueError("%s: the same index twice in one call" % name)
    return np.ascontiguousarray(a, np.int32)


def pair_count(n_a, n_b, default):
    """How many rows a call moves whose two index lists have n_a and n_b entries (None = no list); `default` without any list."""
    if n_a is None and n_b is None:
        return default
    if n_a is not None and n_b is not None and n_a != n_b:
        raise ValueError("index lists of different lengths: %d and %d" % (n_a, n_b))
    return n_a if n_a is not None else n_b


class Snapshot:
    """`capacity` slots of saved env states in the env's device memory.  Belongs to the env that made it (VecNovelGridworld.snapshot);
    closed by close(), by the env's close() and by an in-place rebuild() (inject_novelty) - a closed snapshot raises on use.

    Index arguments: None (0 .. count-1), a list / numpy array of ints (checked on the host - dtype, range, distinct where required -
    and uploaded), or a torch int32 tensor on the env's device (used in place, its VALUES unchecked: an index out of range skips that
    copy and raises the env's sticky F_BAD_INDEX flag; the tensor must be complete before the call - the env runs on its own stream -
    and must not be changed until the env's stream has passed the call)."""

    def __init__(self, env, capacity):
        self.env, self.capacity = env, int(capacity)
        self._s = C.c_void_p()
        self._keep = None                       # uploaded index lists the last call may still be reading
        _cabi.check(_cabi.lib().ngw_snapshot_create(env._h, self.capacity, C.byref(self._s)))

    def _open(self):
        if not self._s or not self.env._h:
            raise ValueError("snapshot is closed")
        return self._s

    def _dev_index(self, idx, limit, distinct, name):
        """-> (device pointer or None, length or None, the uploaded tensor or None)."""
        if idx is None:
            return None, None, None
        import torch
        dev = torch.device('cuda:%d' % self.env.device)
        if isinstance(idx, torch.Tensor):
            if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != dev:
                raise ValueError("%s: a contiguous one-dimensional int32 tensor on %s expected" % (name, dev))
            return idx.data_ptr(), int(idx.numel()), None
        a = check_indices(idx, limit, distinct, name)
        t = torch.from_numpy(a).to(dev)
        return t.data_ptr(), int(a.size), t

    def _call(self, fn, first, second, default_count, *extra):
        import torch
        env = self.env
        count = pair_count(first[1], second[1], default_count)
        uploaded = [t for t in (first[2], second[2]) if t is not None]
        if self._keep:
            env.sync()                          # (the previous call has read its lists: they may be released now)
            self._keep = None
        if uploaded:
            torch.cuda.current_stream(env.device).synchronize()   # the uploads ran on torch's stream, the copy runs on the env's
        _cabi.check(fn(env._h, self._open(), C.c_void_p(first[0]), C.c_void_p(second[0]), int(count), *extra))
        self._keep = uploaded or None

    def save(self, envs=None, slots=None):
        """slot[slots[j]] := state of env envs[j].  The slots of one call must be distinct."""
        self._open()
        e = self._dev_index(envs, self.env.num_envs, False, 'envs')
        s = self._dev_index(slots, self.capacity, True, 'slots')
        self._call(_cabi.lib().ngw_snapshot_save, e, s, self.env.num_envs)

    def restore(self, slots=None, envs=None, keep_episode=False):
        """state of env envs[j] := slot[slots[j]].  Slots may repeat (the fork); the envs of one call must be distinct; envs not named
        keep their state.  keep_episode: the destination envs keep their own episode counters."""
        self._open()
        s = self._dev_index(slots, self.capacity, False, 'slots')
        e = self._dev_index(envs, self.env.num_envs, True, 'envs')
        self.env._lidar_rows_fresh = False
        self._call(_cabi.lib().ngw_snapshot_restore, s, e, self.env.num_envs, KEEP_EPISODE if keep_episode else 0)

    def state(self, first=0, count=None):
        """The saved states of `count` slots from `first`, as get_state() returns them (a never-saved slot: zeros, agent at (1, 1))."""
        self._open()
        count = self.capacity - first if count is None else count
        S2, K = self.env.map_size ** 2, self.env.n_items
        st = {'map': np.zeros((count, S2), np.int8), 'loc': np.zeros((count, 2), np.int32),
              'facing': np.zeros(count, np.int32), 'inv': np.zeros((count, K), np.int32),
              'selected': np.zeros(count, np.int32), 'step_count': np.zeros(count, np.int32),
              'episode': np.zeros(count, np.uint32)}
        _cabi.check(_cabi.lib().ngw_snapshot_get(self.env._h, self._s, first, count, _cabi._ptr(st['map'], np.int8), _cabi._ptr(st['loc'], np.int32),
                                                 _cabi._ptr(st['facing'], np.int32), _cabi._ptr(st['inv'], np.int32),
                                                 _cabi._ptr(st['selected'], np.int32), _cabi._ptr(st['step_count'], np.int32),
                                                 _cabi._ptr(st['episode'], np.uint32)))
        return st

    @property
    def closed(self):
        return not self._s

    def close(self):
        if self._s and self.env._h:
            _cabi.check(_cabi.lib().ngw_snapshot_destroy(self.env._h, self._s))
        self._invalidate()
        snaps = self.env.__dict__.get('_snapshots')
        if snaps and self in snaps:
            snaps.remove(self)

    def _invalidate(self):
        """The handle is gone (or going), and the buffer with it."""
        self._s = C.c_void_p()
        self._keep = None
