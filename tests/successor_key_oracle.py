"""Expected successor keys from the two oracles that exist: the child of (parent, a) is expand_oracle.oracle_expand's - the unmodified CPU oracle's
step -, its key is state_key_oracle.keys_of's - the contract in plain Python integers -, its reports are the same oracle_expand's.  A loop over
a of oracle_expand(..., actions = full(count, a)); nothing here comes from the HIP path (tests/test_successor_keys*.py compare with these).

keys_of hashes one cell at a time, so a field's key is computed once per DISTINCT value of that field among the children (most actions leave the
map as it is) and handed to every child that holds it: the same function on the same bytes, fewer times."""
import functools

import numpy as np

import expand_oracle as XO
import snapshot_oracle as SO
import state_key_oracle as SK
from key_table_oracle import KeyTableModel

COLUMNS = {SK.MAP: ('map',), SK.POSE: ('loc', 'facing'), SK.INV: ('inv',), SK.SELECTED: ('selected',), SK.STEP_COUNT: ('step_count',),
           SK.EPISODE: ('episode',)}
REPORTS = ('reward', 'done', 'result', 'info')


def single_field_keys(rows, bit):
    """uint64 [n]: keys_of(rows, 0 .. n-1, bit), each distinct value of the field's columns hashed once."""
    n = len(rows['map'])
    flat = np.concatenate([np.asarray(rows[k]).reshape(n, -1).astype(np.int64) for k in COLUMNS[bit]], 1)
    _, first, inverse = np.unique(flat, axis=0, return_index=True, return_inverse=True)
    sub = {k: np.asarray(rows[k])[first] for k in COLUMNS[bit]}
    return SK.keys_of(sub, range(len(first)), bit)[np.asarray(inverse).reshape(-1)]


class Successors:
    """The children of every (parent, action) of one call and what the call must return for them.  parents: row indices into `rows` (a dict
    keyed as get_state() keys it, or an oracle State); they may repeat - each distinct parent is stepped once per action."""

    def __init__(self, spec, rows, parents, autoreset=False, horizon=0):
        parents = np.asarray(parents, np.int64)
        self.A = A = len(spec.actions_id)
        uniq, self.inverse = np.unique(parents, return_inverse=True)
        if len(parents) == 0:                                         # (no parent: the oracle has nothing to step; row 0 gives the shapes)
            uniq, self.inverse = np.zeros(1, np.int64), np.zeros(0, np.int64)
        kids, reps = [], []
        for a in range(A):
            k, r = XO.oracle_expand(spec, rows, uniq, np.full(len(uniq), a), autoreset, horizon)
            kids.append(k)
            reps.append(r)
        # [distinct parents * A, ...], row-major: parent p, action a at p * A + a
        self.kids = {k: np.stack([kid[k] for kid in kids], 1).reshape((len(uniq) * A,) + kids[0][k].shape[1:]) for k in XO.STATE_KEYS}
        self.rep = {k: np.stack([r[k] for r in reps], 1)[self.inverse] for k in REPORTS}
        self.singles = {}

    def keys(self, fields):
        """uint64 [count, A]"""
        assert 0 < fields <= SK.ALL
        key = np.zeros(len(self.kids['map']), np.uint64)
        for bit in SK.SINGLE:
            if fields & bit:
                if bit not in self.singles:
                    self.singles[bit] = single_field_keys(self.kids, bit)
                key = key ^ self.singles[bit]
        return key.reshape(-1, self.A)[self.inverse]

    def child_rows(self, pos, actions):
        """The seven arrays of the children of (parents[pos[i]], actions[i])."""
        at = self.inverse[np.asarray(pos, np.int64)] * self.A + np.asarray(actions, np.int64)
        return {k: v[at] for k, v in self.kids.items()}


def assert_successors(got, exp, fields, where, reports=True, zero_rows=()):
    """A SuccessorKeys (numpy or tensors) against a Successors under `fields`; rows in zero_rows must be all zeros in every field instead."""
    keys = SK.as_u64(got.keys)
    want = exp.keys(fields).copy()
    zero = np.zeros(len(want), bool)
    zero[list(zero_rows)] = True
    want[zero] = 0
    assert keys.shape == want.shape, (where, keys.shape, want.shape)
    bad = np.argwhere(keys != want)
    assert len(bad) == 0, "%s, fields %d: %d of %d keys differ, first at parent %d action %d: got %#018x, expected %#018x" % (
        where, fields, len(bad), want.size, bad[0][0], bad[0][1], int(keys[tuple(bad[0])]), int(want[tuple(bad[0])]))
    if not reports:
        assert got.reward is None and got.done is None and got.result is None and got.info is None, where
        return
    host = {k: (got[k].cpu().numpy() if hasattr(got[k], 'data_ptr') else np.asarray(got[k])) for k in REPORTS}
    rep = {k: np.where(zero[:, None], np.zeros((), v.dtype), v) for k, v in exp.rep.items()}
    XO.assert_reports({k: v.reshape(-1) for k, v in host.items()}, {k: v.reshape(-1) for k, v in rep.items()}, where)
    for k in REPORTS:
        assert host[k].shape == want.shape, (where, k, host[k].shape)


class _BoundSuccessorSnapshot(XO._BoundExpandSnapshot):
    """expand_oracle's bound snapshot with Snapshot.successor_keys / insert_successor_keys: the product's host checks (snapshot.check_slots,
    state_keys.check_fields) and bookkeeping (snapshot.insert_successors), the oracles' children and keys."""

    def successor_keys(self, slots=None, fields=SK.STATE, device=False, reports=True):
        from gym_novel_gridworlds_amd.snapshot import SuccessorKeys, check_slots
        from gym_novel_gridworlds_amd.state_keys import check_fields
        self._open()
        f = check_fields(fields)
        s, count = check_slots(slots, self.capacity, None, False, 'slots')
        env = self.env
        ex = Successors(env.spec, self.model.rows, np.arange(count) if s is None else s, env.o.autoreset, env.o.horizon)
        rep = [ex.rep[k] for k in REPORTS] if reports else [None] * 4
        return SuccessorKeys(ex.keys(f), *rep)

    def insert_successor_keys(self, table, slots=None, fields=SK.STATE, device=False):
        import torch
        from gym_novel_gridworlds_amd.snapshot import insert_successors
        s = self.successor_keys(slots, fields)
        as_tensor = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else    # noqa: E731
                                               np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x))
        return insert_successors(type(s)(*[as_tensor(x) for x in s]), table, device)


class ModelKeyTable:
    """KeyTable.insert over key_table_oracle's model: takes what insert_successors hands over (one contiguous one-dimensional int64 tensor) and
    answers as the device table does (`where` is the key's first-seen order here)."""

    def __init__(self):
        self.model, self.calls = KeyTableModel(), []

    def insert(self, keys, device=False):
        import torch
        from gym_novel_gridworlds_amd.key_table import KeyInsert
        assert isinstance(keys, torch.Tensor) and keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
        self.calls.append(int(keys.numel()))
        k = keys.numpy().view(np.uint64)
        fresh, stored = self.model.insert(k)
        where = np.array([self.model.order[int(x)] if s else -1 for x, s in zip(k.tolist(), stored)], np.int32).reshape(len(k))
        return KeyInsert(torch.from_numpy(where), torch.from_numpy(fresh)) if device else KeyInsert(where, fresh)


class OracleVecSuccessors(XO.OracleVecExpand):
    """expand_oracle.OracleVecExpand whose snapshots and envs answer successor_keys: lets the host logic run without a GPU."""

    def snapshot(self, capacity=None):
        s = _BoundSuccessorSnapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s

    def successor_keys(self, envs=None, fields=SK.STATE, device=False, reports=True):
        from gym_novel_gridworlds_amd.snapshot import SuccessorKeys, check_slots
        from gym_novel_gridworlds_amd.state_keys import check_fields
        f = check_fields(fields)
        e, count = check_slots(envs, self.num_envs, None, False, 'envs')
        ex = Successors(self.spec, self.o.st, np.arange(count) if e is None else e, self.o.autoreset, self.o.horizon)
        return SuccessorKeys(ex.keys(f), *([ex.rep[k] for k in REPORTS] if reports else [None] * 4))


sharded_on_oracle = functools.partial(SO.T.sharded_on_oracle, OracleVecSuccessors)


__all__ = ['SO', 'Successors', 'assert_successors', 'single_field_keys', 'OracleVecSuccessors', 'ModelKeyTable', 'sharded_on_oracle']
