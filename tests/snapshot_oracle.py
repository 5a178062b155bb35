"""What a device-side snapshot must do, stated with numpy indexing on arrays shaped like get_state()'s (tests/test_snapshot*.py): a model
of the snapshot buffer that acts on the CPU oracle's State, and oracle-backed stand-ins for the batched and the sharded env with the
snapshot surface.  Nothing here comes from the HIP path."""
import functools

import numpy as np

import ngw_testlib as T

STATE_KEYS = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')


def oracle_state(o):
    """Copies of the oracle's seven state arrays, keyed as get_state() keys them."""
    return {k: getattr(o.st, k).copy() for k in STATE_KEYS}


def put_state(o, st):
    """The oracle's own set_state: the arrays assigned back."""
    for k in STATE_KEYS:
        getattr(o.st, k)[...] = st[k]


class NumpySnapshot:
    """`capacity` slots of the seven arrays; a never-saved slot is the zero row with the agent at (1, 1)."""

    def __init__(self, S, K, capacity):
        self.capacity = capacity
        self.rows = {'map': np.zeros((capacity, S * S), np.int8), 'loc': np.ones((capacity, 2), np.int32), 'facing': np.zeros(capacity, np.int32),
                     'inv': np.zeros((capacity, K), np.int32), 'selected': np.zeros(capacity, np.int32),
                     'step_count': np.zeros(capacity, np.int32), 'episode': np.zeros(capacity, np.uint32)}

    @staticmethod
    def _pair(a, b, default):
        count = default if a is None and b is None else len(a if a is not None else b)
        a = np.arange(count) if a is None else np.asarray(a)
        b = np.arange(count) if b is None else np.asarray(b)
        assert len(a) == len(b)
        return a, b

    def save(self, st, envs=None, slots=None):
        """slot[slots[j]] := state[envs[j]] (st: an oracle State)"""
        e, s = self._pair(envs, slots, st.n)
        for k in STATE_KEYS:
            self.rows[k][s] = getattr(st, k)[e]

    def restore(self, st, slots=None, envs=None, keep_episode=False):
        """state[envs[j]] := slot[slots[j]]; keep_episode: the destination's episode counters stay"""
        s, e = self._pair(slots, envs, st.n)
        for k in STATE_KEYS:
            if not (keep_episode and k == 'episode'):
                getattr(st, k)[e] = self.rows[k][s]

    def state(self, first=0, count=None):
        count = self.capacity - first if count is None else count
        return {k: v[first:first + count].copy() for k, v in self.rows.items()}


class _BoundSnapshot:
    """The Snapshot surface (gym_novel_gridworlds_amd/snapshot.py) over the model, bound to one oracle-backed env."""

    def __init__(self, env, capacity):
        self.env, self.capacity, self.closed = env, capacity, False
        self.model = NumpySnapshot(env.spec.map_size, len(env.spec.items_id), capacity)

    def _open(self):
        if self.closed:
            raise ValueError("snapshot is closed")

    def save(self, envs=None, slots=None):
        self._open()
        self.model.save(self.env.o.st, envs, slots)

    def restore(self, slots=None, envs=None, keep_episode=False):
        self._open()
        self.model.restore(self.env.o.st, slots, envs, keep_episode)

    def state(self, first=0, count=None):
        self._open()
        return self.model.state(first, count)

    def close(self):
        self.closed = True


class OracleVecSnap(T.OracleVec):
    """T.OracleVec with VecNovelGridworld's snapshot() / fork()."""

    def snapshot(self, capacity=None):
        s = _BoundSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s

    def fork(self, src, keep_episode=False):
        s = self.snapshot()
        s.save()
        s.restore(slots=src, keep_episode=keep_episode)
        s.close()

    def rebuild(self, spec):
        for s in self.__dict__.get('_snapshots', ()):
            s.close()
        return super().rebuild(spec)


sharded_on_oracle = functools.partial(T.sharded_on_oracle, OracleVecSnap)
