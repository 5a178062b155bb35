"""Device-side snapshots of a VecNovelGridworld: save, restore and fork env states by index without leaving the GPU
(include/ngw.h ngw_snapshot_*; the kernel is csrc/ngw_snapshot.inc).

    snap = env.snapshot()                      # one slot per env
    snap.save()                                # slot i := env i
    ...
    snap.restore()                             # env i := slot i: the envs are back where they were, episode counters included
    snap.restore(slots=best, envs=worst)       # population methods: the states saved from the best envs over the worst
    env.fork(src)                              # env e := env src[e]
    pool = env.snapshot(4096)                  # a node pool: tree search keeps the states it grows
    e = pool.expand(parents, actions, children)    # slot children[j] := slot parents[j] stepped once with actions[j]; no env is touched
    r = pool.rollout(parents, plans)               # score T-step action sequences from saved slots: ret / length / ended / info, nothing kept
    r = pool.rollout(parents, plans, children)     # ... and keep the state each sequence ends in (a macro-action applied to a node)
    obs = pool.lidar_observation(nodes)            # look at saved slots without restoring them: LidarInFront rows,
    view = pool.agent_view(nodes)                  # ... the AgentMap observation,
    ok = pool.action_masks(nodes)                  # ... and the valid-action masks; no env is touched
    k = pool.keys(nodes)                           # 64-bit state keys: "are these two nodes the same state?" (state_keys.py: the contract)
    first, inverse = pool.unique(nodes)            # ... and the groups of equal states among them
    k, found = pool.insert_keys(table, nodes)      # ... and which of them no earlier call has seen (key_table.py: env.key_table(capacity))
    archive.copy(nodes[found.fresh], free, source=pool)   # slot to slot, unchanged: the new ones move from a scratch pool into an archive pool
    s, found = pool.insert_successor_keys(table, nodes)   # the keys of every action's child, no child stored: expand only fresh_pairs(found.fresh)

What a restored env does next: env e, when it next resets, draws from env e's OWN stream at its (restored or kept) episode counter.  Two
forks of one slot share the rest of the current episode and differ from their next reset on; restoring the same env from the same slot
twice replays the same future.  reward / done / info of the last step are not part of a snapshot."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .state_keys import KEY_STATE, check_fields, unique_of_keys

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


def _check_ids(a, n_actions, name, shape_error):
    """The dtype and range checks check_action_ids and check_plan_ids share; shape_error: None, or what is wrong with a.shape."""
    if a.dtype.kind not in 'iu':
        raise ValueError("%s: integer action ids expected, got dtype %s" % (name, a.dtype))
    if shape_error:
        raise ValueError("%s: %s expected, got shape %s" % (name, shape_error, a.shape))
    bad = (a < 0) | (a >= n_actions)
    if bad.any():
        raise ValueError("%d is not in list" % int(a[bad][0]))
    return np.ascontiguousarray(a, np.int32)


def check_action_ids(actions, n_actions, name='actions'):
    """The host-side check of one action id per pair given as a list / numpy array: integer dtype, one dimension, every id in the action
    list (ValueError("<a> is not in list") otherwise, what step() raises).  Returns a contiguous int32 array."""
    if actions is None:
        raise ValueError("%s: one action id per pair expected" % name)
    a = np.asarray(actions)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int32)            # (an empty list has no dtype of its own)
    return _check_ids(a, n_actions, name, a.ndim != 1 and "a one-dimensional list of action ids")


def check_plan_ids(plans, n_actions, name='plans'):
    """The host-side check of one action sequence per pair given as a list / numpy array [count, T]: integer dtype, two dimensions, at
    least one step, every id in the action list (ValueError("<a> is not in list") otherwise, what step() raises).  Returns a contiguous int32
    array [count, T]."""
    if plans is None:
        raise ValueError("%s: one action sequence per pair expected" % name)
    a = np.asarray(plans)
    if a.ndim == 2 and a.shape[0] == 0 and a.shape[1] >= 1:
        return np.zeros(a.shape, np.int32)      # (an empty list has no dtype of its own)
    return _check_ids(a, n_actions, name, (a.ndim != 2 or a.shape[1] < 1) and "action ids shaped [count, T] with T >= 1")


def _check_pairs(parents, middle, check_middle, children, n_parents, capacity, same_buffer, device_len, children_default):
    """What check_expand and check_rollout share.  middle: the argument between parents and children, checked by check_middle where it is
    no device tensor, or - check_middle None - its length.  children_default: children=None means slots 0 .. count-1 (expand), not "nothing
    is kept" (rollout).  Returns (parents, middle, children, count)."""
    on_dev = device_len or (lambda x: None)
    n_p, n_m, n_c = on_dev(parents), on_dev(middle) if check_middle else middle, on_dev(children)
    host_lists = n_p is None and n_c is None
    if n_p is None and parents is not None:
        parents = check_indices(parents, n_parents, False, 'parents')
        n_p = int(parents.size)
    if n_m is None:
        middle = check_middle(middle)
        n_m = int(middle.size)
    if n_c is None and children is not None:
        children = check_indices(children, capacity, True, 'children')
        n_c = int(children.size)
    count = pair_count(pair_count(n_p, n_m, n_m), n_c, n_m)
    kept = children_default or children is not None
    if parents is None and count > n_parents:
        raise ValueError("parents: no list given and %d pairs for %d rows" % (count, n_parents))
    if kept and count > capacity:
        raise ValueError("children: %d pairs for a snapshot of %d slots" % (count, capacity))
    if same_buffer and count and kept and host_lists:
        hp = np.arange(count) if parents is None else parents
        hc = np.arange(count) if children is None else children
        both = np.intersect1d(hp, hc)
        if both.size:
            raise ValueError("children: slot %d is also a parent of the same call (source and destination are one buffer)" % int(both[0]))
    return parents, middle, children, count


def check_expand(parents, actions, children, n_parents, capacity, n_actions, same_buffer, device_len=None):
    """The host-side checks of one expand call: parents index rows [0, n_parents) and may repeat, children index slots [0, capacity) and
    must be distinct, actions are ids of the action list, the three have one length (None = no list: 0 .. count-1, which must exist), and -
    where source and destination are the same buffer - no child is also a parent.  device_len(x): the length of x when it is a device
    tensor to be used in place (its values are then not checked), else None.  Returns (parents, actions, children, count): contiguous
    int32 arrays, None, or the device tensors themselves."""
    return _check_pairs(parents, actions, lambda a: check_action_ids(a, n_actions), children, n_parents, capacity, same_buffer, device_len, True)


def check_rollout(parents, n_plans, children, n_parents, capacity, same_buffer, device_len=None):
    """The host-side checks of one rollout call's index lists: parents index rows [0, n_parents) and may repeat (None = 0 .. count-1, which
    must exist); children - None: nothing is kept - index slots [0, capacity) and must be distinct; both have the plans' length n_plans,
    and - where source and destination are the same buffer - no child is also a parent.  device_len(x): the length of x when it is a
    device tensor to be used in place (its values are then not checked), else None.  Returns (parents, children, count): contiguous int32
    arrays, None, or the device tensors themselves."""
    p, _, c, count = _check_pairs(parents, n_plans, None, children, n_parents, capacity, same_buffer, device_len, False)
    return p, c, count


def check_playout(parents, steps, children, n_parents, capacity, same_buffer, device_len=None):
    """The host-side checks of one playout call: `steps` is an integer >= 1, and the index lists are a rollout's (check_rollout) - with no
    plans to count the pairs, the number of pairs is the length of parents, or of children where parents is None (0 .. count-1).  Returns
    (parents, children, count, steps)."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
        raise ValueError("steps: an integer number of steps expected, got %r" % (steps,))
    if steps < 1:
        raise ValueError("steps: at least one step expected, got %d" % steps)
    given = parents if parents is not None else children
    if given is None:
        raise ValueError("parents: without parents and children the number of pairs is not known")
    n = None if device_len is None else device_len(given)
    if n is None:
        n = len(given)
    p, c, count = check_rollout(parents, int(n), children, n_parents, capacity, same_buffer, device_len)
    return p, c, count, int(steps)


def check_limits(limits, count, steps, device_len=None):
    """The host-side check of the per-pair step limits of a rollout / playout: None; a list / numpy array of `count` integers in [0, steps]
    (ValueError otherwise) -> a contiguous int32 array; or - device_len(x) gives its length - a device int32 tensor of `count` elements, used
    in place with its VALUES unchecked (the kernel clamps them to [0, steps])."""
    if limits is None:
        return None
    n = None if device_len is None else device_len(limits)
    if n is None:
        a = np.asarray(limits)
        if a.ndim != 1 or (a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer))):
            raise ValueError("limits: a one-dimensional list of integers expected")
        if a.size and (a.min() < 0 or a.max() > steps):
            bad = a[(a < 0) | (a > steps)][0]
            raise ValueError("limits: %d outside [0, %d]" % (int(bad), steps))
        limits, n = np.ascontiguousarray(a, dtype=np.int32), int(a.size)
    if n != count:
        raise ValueError("limits: %d limits for %d pairs" % (n, count))
    return limits


def check_copy(src_slots, dst_slots, n_src, capacity, same_buffer, device_len=None):
    """The host-side checks of one slot-to-slot copy, as check_expand checks children: src_slots index rows [0, n_src) and may repeat,
    dst_slots index slots [0, capacity) and must be distinct, both have one length (None = no list: 0 .. count-1, which must exist; without
    any list: every slot of the source), and - where source and destination are the same buffer - no destination is also a source.
    device_len as in check_expand.  Returns (src_slots, dst_slots, count)."""
    on_dev = device_len or (lambda x: None)
    n_s, n_d = on_dev(src_slots), on_dev(dst_slots)
    host_lists = n_s is None and n_d is None
    if n_s is None and src_slots is not None:
        src_slots = check_indices(src_slots, n_src, False, 'src_slots')
        n_s = int(src_slots.size)
    if n_d is None and dst_slots is not None:
        dst_slots = check_indices(dst_slots, capacity, True, 'dst_slots')
        n_d = int(dst_slots.size)
    count = pair_count(n_s, n_d, int(n_src))
    if src_slots is None and count > n_src:
        raise ValueError("src_slots: no list given and %d pairs for %d slots" % (count, n_src))
    if count > capacity:
        raise ValueError("dst_slots: %d pairs for a snapshot of %d slots" % (count, capacity))
    if same_buffer and count and host_lists:
        hs = np.arange(count) if src_slots is None else src_slots
        hd = np.arange(count) if dst_slots is None else dst_slots
        both = np.intersect1d(hs, hd)
        if both.size:
            raise ValueError("dst_slots: slot %d is also a source of the same call (source and destination are one buffer)" % int(both[0]))
    return src_slots, dst_slots, count


def check_slots(slots, capacity, device_len=None, distinct=False, name='slots'):
    """The host-side checks of one index list that reads or writes rows [0, capacity) (the slot observations, the state keys, save / restore):
    None = every row, 0 .. capacity-1; a list / numpy array may repeat unless `distinct` (its length is not bound by the capacity).
    device_len(x): the length of x when it is a device tensor to be used in place (its values are then not checked), else None.  Returns
    (slots, count): a contiguous int32 array, None, or the device tensor itself."""
    if slots is None:
        return None, int(capacity)
    n = None if device_len is None else device_len(slots)
    if n is not None:
        return slots, int(n)
    slots = check_indices(slots, capacity, distinct, name)
    return slots, int(slots.size)


def tensor_len(dev, name, x, dtype='int32'):
    """The one check of an argument that may be a device tensor used in place: the length of x when it is a contiguous one-dimensional
    torch tensor of `dtype` (int32: an index list; int64: a key list) on `dev` (the env's torch device), None when it is no tensor, ValueError
    for any other tensor."""
    import torch
    if not isinstance(x, torch.Tensor):
        return None
    if x.dtype != getattr(torch, dtype) or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
        raise ValueError("%s: a contiguous one-dimensional %s tensor on %s expected" % (name, dtype, dev))
    return int(x.numel())


def upload(dev, count, *args):
    """The checked arguments of one call (None, numpy arrays, device tensors) -> ([a device pointer each; None for None and where count is 0],
    [the tensors uploaded here]).  The only place a host array becomes a device tensor."""
    import torch
    ptrs, uploaded = [], []
    for x in args:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x).to(dev)
            uploaded.append(x)
        ptrs.append(C.c_void_p(x.data_ptr()) if x is not None and count else None)
    return ptrs, uploaded


def index_arg(env, idx, limit, name, distinct=False):
    """One index list of a call that moves or reads rows by index (save / restore, the slot observations, the state keys), checked and
    uploaded: None, a list / numpy array (check_indices) or a contiguous torch int32 tensor on the env's device, used in place.
    -> (device pointer or None, count - `limit` without a list -, torch device, [the uploaded tensor] or [])."""
    import torch
    dev = torch.device('cuda:%d' % env.device)
    s, count = check_slots(idx, limit, lambda x: tensor_len(dev, name, x), distinct, name)
    (ptr,), uploaded = upload(dev, count, s)
    return ptr, count, dev, uploaded


def enqueue_ordered(env, holder, call, count, uploaded, device, behind=True):
    """One launch on the env's stream that reads and writes torch tensors: the env's stream waits for torch's current one (uploads, the
    allocations of the outputs, the caller's own tensors) unless that stream has finished all its work, and behind the launch either torch's stream waits for the env's (device=True: no
    host wait) or the host does - or, behind=False (a call without outputs: save / restore), nothing does.  `holder._keep` keeps the
    uploaded lists alive until the next call of the holder has synchronised."""
    import torch
    if holder._keep:
        env.sync()                              # (the previous call has read its lists: they may be released now)
        holder._keep = None
    if count:
        ahead = torch.cuda.current_stream(env.device)
        if not ahead.query():                   # (an idle stream has nothing to wait for: the wait alone costs a restore + step + save loop 40 %)
            env.stream_order(ahead.cuda_stream, True)
        _cabi.check(call())
        holder._keep = uploaded or None
    if not behind:
        return
    if device:
        if count:
            env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, False)
    else:
        env.sync()
        holder._keep = None


class Expansion(collections.namedtuple('Expansion', 'reward done result info')):
    """What Snapshot.expand() returns: reward int32, done bool, result bool and info uint32 (the packed words: decode_info_words(e.info)
    gives what step_costs() / messages() take), each [count] - what step() would have reported for each pair.  A named tuple (it unpacks
    in that order) whose fields can also be read by name: e['reward'].  numpy arrays, or torch tensors ('info' is int32 there, the same bits)."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    @property
    def goal(self):
        """The step itself reported done (info bit 1, as on PlanEval: set by the goal - and by a FireWall death, which `died` tells
        apart -, clear for a horizon cut)."""
        return self.done & (((self.info >> 1) & 1) != 0)

    @property
    def died(self):
        """The step ended the episode in a FireWall death (message code 14)."""
        return self.done & (((self.info >> 8) & 255) == 14)

    def reshape(self, *shape):
        return Expansion(*[x.reshape(*shape) for x in self])


def all_actions_pairs(parents, first_child, n_actions):
    """expand_all's index arithmetic: every parent paired with every action id 0 .. A-1, the children in len(parents) * A consecutive slots
    from first_child (row-major: parent p, action a -> slot first_child + p * A + a).  parents: a list / numpy array, or a torch tensor
    (the three lists are then tensors on its device).  -> (parents, actions, children, (P, A))"""
    A = int(n_actions)
    if hasattr(parents, 'data_ptr'):
        import torch
        P = int(parents.numel())
        ids = torch.arange(P * A, dtype=torch.int32, device=parents.device)
        return parents.repeat_interleave(A).contiguous(), (ids % A).contiguous(), ids + int(first_child), (P, A)
    p = np.asarray(parents)
    P = int(p.size)
    ids = np.arange(P * A, dtype=np.int64)
    return np.repeat(p, A), ids % A, ids + int(first_child), (P, A)


class SuccessorKeys(collections.namedtuple('SuccessorKeys', 'keys reward done result info')):
    """What successor_keys() returns, each [count, A]: 'keys' - entry (j, a) the key of the child an expand of parent j with action a would
    write, numpy uint64 or a torch int64 tensor over the same bits - and the Expansion fields of that expand: 'reward' int32, 'done' bool,
    'result' bool, 'info' uint32 (int32 as a tensor).  With reports=False the four report fields are None.  Fields by name too: s['keys']."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    @property
    def goal(self):
        """Expansion.goal of every (parent, action)."""
        return Expansion.goal.fget(self)

    @property
    def died(self):
        """Expansion.died of every (parent, action)."""
        return Expansion.died.fget(self)


def fresh_pairs(fresh):
    """The (parent position, action id) of every True of a [count, A] `fresh` (insert_successor_keys), in row-major order - the order of the
    flattened keys, so position j * A + a maps back by divmod.  numpy arrays (int64), or torch tensors for a tensor."""
    A = int(fresh.shape[1])
    if hasattr(fresh, 'data_ptr'):
        import torch
        pos = torch.nonzero(fresh.reshape(-1)).reshape(-1)
        return torch.div(pos, A, rounding_mode='floor'), pos % A
    return divmod(np.flatnonzero(np.asarray(fresh).reshape(-1)), A)


def fresh_steps(fresh):
    """The (step t, pair j) of every True of a [T, count] `fresh` (the flattened path keys of a rollout / playout offered to
    KeyTable.insert), in row-major order - position t * count + j maps back by divmod, so a fresh key names the EARLIEST step that reached
    its state.  numpy arrays (int64), or torch tensors for a tensor.  limits = t + 1 replays pair j up to that state."""
    n = int(fresh.shape[1])
    if hasattr(fresh, 'data_ptr'):
        import torch
        pos = torch.nonzero(fresh.reshape(-1)).reshape(-1)
        return torch.div(pos, n, rounding_mode='floor'), pos % n
    return divmod(np.flatnonzero(np.asarray(fresh).reshape(-1)), n)


def transitions(result):
    """The (step t, pair j) of every step a rollout / playout result executed - t < length[j] -, in row-major order (all pairs of step 0, then of
    step 1, ...): numpy arrays (int64), or torch tensors for a result on the device.  With them a dataset is three gathers:
    obs[t, j], actions[t, j], rewards[t, j] -> obs[t + 1, j] (an [N, P] result: j numbers its pairs row-major, reshape the fields to [T, N * P]).
    T is read off the first per-step field the result holds."""
    length = result.length
    steps = None
    for name in ('rewards', 'masks', 'keys', 'actions', 'obs'):
        x = getattr(result, name, None)
        if x is not None:
            x = x[0] if isinstance(x, tuple) else (next(iter(x.values())) if isinstance(x, dict) else x)
            steps = int(x.shape[0]) - (1 if name == 'obs' else 0)
            break
    if steps is None:
        raise ValueError("transitions: the result holds no per-step field")
    if hasattr(length, 'data_ptr'):
        import torch
        ran = torch.arange(steps, device=length.device)[:, None] < length.reshape(1, -1)
        pos = torch.nonzero(ran.reshape(-1)).reshape(-1)
        n = max(int(length.numel()), 1)
        return torch.div(pos, n, rounding_mode='floor'), pos % n
    length = np.asarray(length).reshape(-1)
    ran = np.arange(steps)[:, None] < length[None, :]
    return divmod(np.flatnonzero(ran.reshape(-1)), max(int(length.size), 1))


VIEW_SIZE_MAX = 16        # include/ngw.h NGW_TRAJ_VIEW_MAX


def check_observe(env, observe, view_size=5):
    """The `observe` and `view_size` keywords of a rollout / playout: None -> False; 'lidar' on an env with a lidar configured -> True;
    'agent_view' (no lidar needed) with an integer view_size in 1 .. VIEW_SIZE_MAX -> 'agent_view'.  view_size belongs to 'agent_view': with any
    other `observe` it stays at its default.  Everything else is a ValueError, before a handle is touched."""
    default = isinstance(view_size, (int, np.integer)) and not isinstance(view_size, bool) and view_size == 5
    if isinstance(observe, str) and observe == 'agent_view':
        if isinstance(view_size, bool) or not isinstance(view_size, (int, np.integer)) or not 1 <= view_size <= VIEW_SIZE_MAX:
            raise ValueError("view_size: an integer in 1..%d expected, got %r" % (VIEW_SIZE_MAX, view_size))
        return 'agent_view'
    if observe is not None and not (isinstance(observe, str) and observe == 'lidar'):
        raise ValueError("observe: None or 'lidar' or 'agent_view' expected, got %r" % (observe,))
    if not default:
        raise ValueError("view_size=%r without observe='agent_view': the window belongs to the AgentMap observation" % (view_size,))
    if observe is None:
        return False
    if env.lidar is None:
        refused = getattr(env, 'lidar_refused', None)    # (lidar_configure found the maps too large for the observation's LDS layout, and said so)
        if refused:
            raise MapsTooLarge("map_size %d: observe='lidar' keeps a wavefront's 64 maps in the lidar observation's LDS layout, which this env cannot "
                               "hold - %s; rewards / masks alone keep the path form's limit" % (env.map_size, refused))
        raise ValueError("observe='lidar' before env.lidar_configure (LidarInFront)")
    return True


def traj_outputs(env, dev, rewards, masks, observe, count, steps, view_size=5):
    """What a trajectory call adds to a path call -> (rewards int32 [steps, count] or None, masks int64 [steps, count] or None, the row buffer
    [steps + 1, count rounded up to 64, row] or None - a wave stores whole 64-row tiles, as in lidar_observation -, its stride in rows).  Only what
    was asked for is allocated; the rows take (steps + 1) * pad * row bytes of device memory.  observe: check_observe's result; 'agent_view' makes
    the row buffer the dict of Snapshot.agent_view, every value [steps + 1, pad, ...]."""
    import torch
    rew = torch.zeros((steps, count), dtype=torch.int32, device=dev) if rewards else None
    msk = torch.zeros((steps, count), dtype=torch.int64, device=dev) if masks else None
    rows, pad = None, (count + 63) // 64 * 64
    if observe == 'agent_view':
        W = 2 * int(view_size) + 1
        rows = {'agent_map': torch.empty((steps + 1, pad, W, W), dtype=torch.int8, device=dev),           # (every row of every block is written: whole tiles)
                'agent_facing_id': torch.empty((steps + 1, pad), dtype=torch.int32, device=dev),
                'inventory_items_quantity': torch.empty((steps + 1, pad, env.n_items), dtype=torch.int32, device=dev)}
    elif observe:
        if env.lidar_packed:
            shape, dtype = (steps + 1, pad, env.lidar_row_bytes), torch.uint8
        else:
            shape, dtype = (steps + 1, pad, env.lidar_len), torch.int32 if env.lidar_dtype == np.dtype(np.int32) else torch.int16
        rows = torch.empty(shape, dtype=dtype, device=dev)           # (every row of every block is written: whole tiles)
    return rew, msk, rows, pad


def host(x, view=None):
    """One device result as the host's: a numpy array, its bits seen as `view` where one is given (uint8 -> bool, int32 -> uint32, int64 -> uint64);
    None stays None."""
    if x is None:
        return None
    x = x.cpu().numpy()
    return x if view is None else x.view(view)


def traj_results(env, rew, msk, rows, count, device):
    """The three buffers as the result's fields: on the device as they are (the rows cut to `count` per block), else numpy; packed rows split."""
    if isinstance(rows, dict):                           # (observe='agent_view')
        rows = {k: x[:, :count] for k, x in rows.items()}
        return (rew, msk, rows) if device else (host(rew), host(msk, np.uint64), {k: host(x) for k, x in rows.items()})
    if rows is not None:
        rows = rows[:, :count]
    if not device:
        rew, msk, rows = host(rew), host(msk, np.uint64), host(rows)
    if rows is not None and env.lidar_packed:            # (env._lidar_split, over the last axis)
        beams, tail = rows[..., :env.lidar.num_beams * len(env.lidar.lidar_items_id)], rows[..., env._lidar_inv_off:]
        if isinstance(tail, np.ndarray):
            rows = (beams, tail.view(np.int16))
        else:
            import torch
            rows = (beams, tail.view(torch.int16))
    return rew, msk, rows


def _ptr(x, count):
    return C.c_void_p(x.data_ptr()) if x is not None and count else None


def path_outputs(dev, limits, path_keys, fields, count, steps):
    """What a path call adds to a plain one -> (the checked limits, the fields word, the keys tensor [steps, count] int64 or None)."""
    import torch
    lim = check_limits(limits, count, steps, lambda x: tensor_len(dev, 'limits', x))
    if not path_keys:
        return lim, 0, None
    return lim, check_fields(KEY_STATE if fields is None else fields), torch.zeros((steps, count), dtype=torch.int64, device=dev)


def path_call(env, holder, call, count, uploaded, device):
    """enqueue_ordered for a path call: the library's map-size refusal is MapsTooLarge, as for successor_keys."""
    try:
        enqueue_ordered(env, holder, call, count, uploaded, device)
    except ValueError as e:
        if str(e).startswith('map_size'):
            raise MapsTooLarge(str(e)) from None
        raise


def pairs_call(env, holder, kind, src, dst, parents, children, count, steps, device, plans=None, seed=0, first_pair=0, record=False, weights=None, limits=None,
               path_keys=False, fields=None, rewards=False, masks=False, observe=None, view_size=5, table=None, table_weights=None, guide=None):
    """The one launch behind Snapshot.rollout (kind 'rollout': `plans` the checked step-major [steps, count] actions), Snapshot.playout and
    VecNovelGridworld.playouts (kind 'playout': seed / first_pair / record, and weights: None - the uniform rule - or one float32 per action from the
    host or the device, sample.check_weights).  src / dst are snapshots' C handles (src None: the envs' current states; dst None: nothing is kept),
    parents / children the checked lists (check_rollout / check_playout); `holder` keeps the uploaded lists alive.  limits / path_keys / fields: the
    path form; rewards / masks / observe / view_size: the trajectory form - `observe` has been through check_observe at the caller (before it touched
    a handle).  table / table_weights / guide: the guided form of a playout - `guide` is playout.check_guide's answer (made at the caller, before it touched a
    handle), None without a table; the result is then a PlayoutGuided.  The entry point is playout.pairs_symbol's.  -> PlanEval / RolloutPath (with path_keys) / RolloutTraj, or Playout (actions [steps, count] with
    `record`) / PlayoutPath / PlayoutTraj, as the callers' docstrings define them."""
    import torch
    from .playout import Playout, PlayoutGuided, PlayoutPath, PlayoutTraj, check_table_weights, pairs_symbol
    from .vec_env import PlanEval, RolloutPath, RolloutTraj
    draws = kind == 'playout'
    guided = guide is not None
    traj = guided or observe is not None or bool(rewards) or bool(masks)
    path = traj or limits is not None or bool(path_keys)
    views = isinstance(observe, str) and observe == 'agent_view'
    name = pairs_symbol(kind, weights is not None, path, traj, views, guided)
    seed, first_pair = int(seed), int(first_pair)
    if not 0 <= seed < 1 << 64:                 # (refused before anything is uploaded or allocated)
        raise ValueError("seed: %d outside [0, 2^64)" % seed)
    if not 0 <= first_pair < 1 << 64:
        raise ValueError("first_pair: %d outside [0, 2^64)" % first_pair)
    dev = torch.device('cuda:%d' % env.device)
    ptr, uploaded = upload(dev, count, parents, children, plans)
    ret, length, info = [torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(3)]
    ended = torch.zeros(count, dtype=torch.uint8, device=dev)
    reports = [C.c_void_p(x.data_ptr()) for x in (ret, length, ended, info)]
    first = actions = keys = rew = msk = rows = where = depth = None
    if guided:                                  # (the rows: checked and uploaded before anything is enqueued)
        tw, mine = check_table_weights(table_weights, table.buckets, env.n_actions, dev)
        uploaded = uploaded + ([tw] if mine else [])
    if draws:
        wt = []
        if weights is not None:
            from .sample import check_weights
            w, mine = check_weights(weights, count, env.n_actions, dev, per_pair=False)
            uploaded, wt = uploaded + ([w] if mine else []), [C.c_void_p(w.data_ptr())]
        elif path:
            wt = [None]                         # (only the plain unweighted entry point has no weights argument)
        first = torch.full((count,), -1, dtype=torch.int32, device=dev)
        actions = torch.full((steps, count), -1, dtype=torch.int32, device=dev) if record else None
        head = [env._h, src, ptr[0], int(count), steps, seed, first_pair] + wt
        tail = [dst, ptr[1]] + reports + [C.c_void_p(first.data_ptr()), _ptr(actions, count), int(count)]
    else:
        head = [env._h, src, ptr[0], ptr[2], int(count), steps]
        tail = [dst, ptr[1], int(count)] + reports
    if path:
        lim, f, keys = path_outputs(dev, limits, path_keys, fields, count, steps)
        if guided:
            f = guide[1]                        # (the look-up's selection, keys recorded or not)
        (lim_ptr,), up = upload(dev, count, lim)
        uploaded, head, tail = uploaded + up, head + [lim_ptr], tail + [f, _ptr(keys, count), int(count)]
    if traj:
        rew, msk, rows, pad = traj_outputs(env, dev, rewards, masks, 'agent_view' if views else observe is not None, count, steps, view_size)
        tail += [_ptr(rew, count), int(count)] + ([_ptr(msk, count), int(count)] if draws else [])
        if views:                                        # (the lidar rows' place stays empty; the three buffers travel in one struct)
            vw = _cabi.TrajViews(int(view_size), *[x.data_ptr() for x in (rows['agent_map'], rows['agent_facing_id'], rows['inventory_items_quantity'])], int(pad))
            tail += [None, 0, C.byref(vw) if count else None]
        else:
            tail += [_ptr(rows, count), int(pad)] + ([None] if guided else [])
    if guided:
        where = torch.full((steps, count), -1, dtype=torch.int32, device=dev)
        depth = torch.zeros(count, dtype=torch.int32, device=dev)
        tail += [table._open(), C.c_void_p(tw.data_ptr()), _ptr(where, count), int(count), _ptr(depth, count), guide[0]]
    (path_call if path else enqueue_ordered)(env, holder, lambda: getattr(_cabi.lib(), name)(*head, *tail), count, uploaded, device)
    if count == 0 and rows is not None:
        for x in (rows.values() if views else [rows]):
            x.zero_()
    if device:
        res = [ret, length, ended.view(torch.bool), info] + ([first, actions] if draws else [])
    else:
        res = [host(ret), host(length), host(ended, np.bool_), host(info, np.uint32)] + ([host(first), host(actions)] if draws else [])
        keys = host(keys, np.uint64)
    if traj:
        rew, msk, rows = traj_results(env, rew, msk, rows, count, device)
        if guided:
            return PlayoutGuided(*res, keys, rew, msk, rows, where if device else host(where), depth if device else host(depth))
        return PlayoutTraj(*res, keys, rew, msk, rows) if draws else RolloutTraj(*res, keys, rew, rows)
    plain, keyed = (Playout, PlayoutPath) if draws else (PlanEval, RolloutPath)
    return plain(*res) if keys is None else keyed(*res, keys)


class MapsTooLarge(_cabi.NgwError, ValueError):
    """successor_keys on a handle whose maps the call cannot hold: the library's refusal (NGW_E_INVALID_ARG, a ValueError as every argument
    error is) - and an NgwError, because no argument of the call is wrong: the handle cannot serve it."""


def successor_keys_call(env, holder, s, idx, limit, name, fields, device, reports):
    """The one launch behind Snapshot.successor_keys (s: the snapshot's C handle) and VecNovelGridworld.successor_keys (s None: the envs'
    current states): idx indexes rows [0, limit); `holder` keeps an uploaded list alive.  -> SuccessorKeys."""
    import torch
    f = check_fields(fields)
    ptr, count, dev, uploaded = index_arg(env, idx, limit, name)
    A = env.n_actions
    keys = torch.empty((count, A), dtype=torch.int64, device=dev)
    reward = torch.empty((count, A), dtype=torch.int32, device=dev) if reports else None
    done = torch.empty((count, A), dtype=torch.uint8, device=dev) if reports else None
    info = torch.empty((count, A), dtype=torch.int32, device=dev) if reports else None
    p = [None if x is None else C.c_void_p(x.data_ptr()) for x in (keys, reward, done, info)]
    try:
        enqueue_ordered(env, holder, lambda: _cabi.lib().ngw_successor_keys(env._h, s, ptr, count, f, *p), count, uploaded, device)
    except ValueError as e:
        if str(e).startswith('map_size'):
            raise MapsTooLarge(str(e)) from None
        raise
    if reports:
        succ = SuccessorKeys(keys, reward, done.view(torch.bool), (info & 1).bool(), info)
    else:
        succ = SuccessorKeys(keys, None, None, None, None)
    return succ if device else successors_to_host(succ)


def successors_to_host(succ):
    """A SuccessorKeys of device tensors as numpy arrays (keys uint64, info uint32: the same bits)."""
    host = lambda x, view=None: None if x is None else (x.cpu().numpy() if view is None else x.cpu().numpy().view(view))   # noqa: E731
    return SuccessorKeys(host(succ.keys, np.uint64), host(succ.reward), host(succ.done), host(succ.result), host(succ.info, np.uint32))


def insert_successors(succ, table, device):
    """insert_successor_keys behind the launch: succ (device tensors [count, A]) with its keys flattened row-major into table.insert - no
    host wait in between -, where / fresh reshaped back to [count, A].  -> (SuccessorKeys as `device` asks, KeyInsert)."""
    from .key_table import KeyInsert
    shape = tuple(succ.keys.shape)
    found = table.insert(succ.keys.reshape(-1), device=device)
    return (succ if device else successors_to_host(succ)), KeyInsert(found.where.reshape(shape), found.fresh.reshape(shape))


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

    def _copy(self, fn, src, n_src, src_name, dst, n_dst, dst_name, *extra):
        """save / restore: fn copies row src[j] to row dst[j] (None: 0 .. count-1; the destinations distinct); ordered as restore() says."""
        env = self.env
        self._open()
        p_src, c_src, _, up_src = index_arg(env, src, n_src, src_name)
        p_dst, c_dst, _, up_dst = index_arg(env, dst, n_dst, dst_name, distinct=True)
        count = pair_count(None if src is None else c_src, None if dst is None else c_dst, env.num_envs)
        enqueue_ordered(env, self, lambda: fn(env._h, self._s, p_src, p_dst, count, *extra), count, up_src + up_dst, True, behind=False)

    def save(self, envs=None, slots=None):
        """slot[slots[j]] := state of env envs[j].  The slots of one call must be distinct.  Ordered as restore() is."""
        self._copy(_cabi.lib().ngw_snapshot_save, envs, self.env.num_envs, 'envs', slots, self.capacity, 'slots')

    def restore(self, slots=None, envs=None, keep_episode=False):
        """state of env envs[j] := slot[slots[j]].  Slots may repeat (the fork); the envs of one call must be distinct; envs not named
        keep their state.  keep_episode: the destination envs keep their own episode counters.
        No host wait: the copy runs on the env's stream, which first waits for torch's current stream (an uploaded list, an index tensor
        computed there).  Torch's stream is NOT ordered behind the copy (that edge made a restore + step + save loop several times
        slower): an index tensor must stay unchanged until the env's stream has passed the call, as the class says."""
        self.env._lidar_rows_fresh = False
        self._copy(_cabi.lib().ngw_snapshot_restore, slots, self.capacity, 'slots', envs, self.env.num_envs, 'envs', KEEP_EPISODE if keep_episode else 0)

    def copy(self, src_slots, dst_slots, source=None):
        """slot[dst_slots[j]] := slot[src_slots[j]] of `source` (another Snapshot of the same env; default: this one), unchanged: the whole
        row, episode counter included - a search moves the children that turned out to be new from a scratch pool into an archive pool
        without restoring them into envs.  Sources may repeat; the destinations of one call must be distinct, and inside one buffer no
        destination may also be a source.  Lists and numpy arrays are checked here, as expand() checks children; torch int32 tensors on the
        env's device are used in place, unchecked: an index out of range skips that copy (F_BAD_INDEX).  None means 0 .. count-1 (without
        any list: every slot of the source).  Ordered like save(): no host wait, torch's stream is not ordered behind the copy."""
        import torch
        env = self.env
        src, n_src, same_buffer = self._source(source, False, 'copy')
        dev = torch.device('cuda:%d' % env.device)
        s, d, count = check_copy(src_slots, dst_slots, n_src, self.capacity, same_buffer, lambda x: tensor_len(dev, 'copy', x))
        ptr, uploaded = upload(dev, count, s, d)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_snapshot_copy(env._h, src, ptr[0], self._s, ptr[1], int(count)), count, uploaded, True,
                        behind=False)

    def _source(self, source, from_envs, what):
        """Where the parents of one `what` (expand / rollout) call live -> (the source snapshot's C handle - None: the env's current states -,
        n_parents, whether source and destination are one buffer)."""
        self._open()
        if source is not None and from_envs:
            raise ValueError("%s: give either source or from_envs" % what)
        if from_envs:
            return None, self.env.num_envs, False
        src = self if source is None else source
        if not isinstance(src, Snapshot):
            raise ValueError("source: a Snapshot expected")
        src._open()
        if src.env is not self.env:
            raise ValueError("source: a snapshot of another env")
        return src._s, src.capacity, src is self

    def expand(self, parents, actions, children, from_envs=False, source=None, device=False):
        """slot[children[j]] := the state of parent parents[j] stepped ONCE with actions[j], as the step leaves it before any reset (the
        child of a step that ends the episode is the state the episode ended in; its episode counter is the parent's).  The parents are
        slots of `source` (another Snapshot of the same env; default: this one) or, with from_envs=True, the env's current states.
        Returns an Expansion of what step() would have reported for each pair: 'reward' int32, 'done' bool, 'result' bool, 'info' uint32,
        each [count].  Nothing is committed: no env, no mask, no lookahead table, no prepared episode and no slot but the children changes,
        and the number of pairs is not bound by num_envs.  One kernel launch.
        Parents may repeat (the fan-out); the children of one call must be distinct, and where source and destination are one buffer no
        child may also be a parent of the same call.  Lists and numpy arrays are checked here (range, distinct children, children disjoint
        from parents, action ids - a bad id raises the ValueError step() raises); torch int32 tensors on the env's device are used in place,
        unchecked: an index out of range skips that pair (F_BAD_INDEX, its reports stay 0), an id outside the action list leaves the child a
        copy of the parent with reports 0 (F_INVALID_ACTION), see error_flags().  None for parents or children means 0 .. count-1.
        device=True: the results as torch tensors on the env's device ('info' int32), ordered behind the launch on torch's current stream -
        no copy, no host wait; otherwise numpy arrays after one sync."""
        import torch
        env = self.env
        src, n_parents, same_buffer = self._source(source, from_envs, 'expand')
        dev = torch.device('cuda:%d' % env.device)
        p, a, c, count = check_expand(parents, actions, children, n_parents, self.capacity, env.n_actions, same_buffer,
                                      lambda x: tensor_len(dev, 'expand', x))
        ptr, uploaded = upload(dev, count, p, a, c)
        reward = torch.zeros(count, dtype=torch.int32, device=dev)
        done = torch.zeros(count, dtype=torch.uint8, device=dev)
        info = torch.zeros(count, dtype=torch.int32, device=dev)
        enqueue_ordered(env, self, lambda: _cabi.lib().ngw_snapshot_expand(
            env._h, src, ptr[0], ptr[1], self._s, ptr[2], int(count), C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()),
            C.c_void_p(info.data_ptr())), count, uploaded, device)
        if device:
            return Expansion(reward, done.view(torch.bool), (info & 1).bool(), info)
        words = info.cpu().numpy().view(np.uint32)
        return Expansion(reward.cpu().numpy(), done.cpu().numpy().view(np.bool_), (words & 1).astype(np.bool_), words)

    def expand_all(self, parents, first_child, from_envs=False, source=None, device=False):
        """Every parent with every action id 0 .. A-1 (A = env.n_actions): the child of (parents[p], a) goes to slot first_child + p * A + a.
        Returns the Expansion shaped [len(parents), A]."""
        p, a, c, shape = all_actions_pairs(parents, first_child, self.env.n_actions)
        return self.expand(p, a, c, from_envs=from_envs, source=source, device=device).reshape(*shape)

    def rollout(self, parents, plans, children=None, from_envs=False, source=None, device=False, limits=None, path_keys=False, fields=KEY_STATE,
                rewards=False, masks=False, observe=None, view_size=5):
        """Pair j: the state of parent parents[j] stepped on a private copy with the T actions of plans[j], by the rules evaluate_plans()
        applies - every novelty, the env's autoreset setting and horizon; it stops at the first step that ends the episode (goal, FireWall
        death, the horizon under autoreset), that step counts, and no reset ever runs.  Returns a PlanEval of 'ret' int32 (sum of the
        executed steps' rewards), 'length' int32 (steps executed, 1 .. T), 'ended' bool and 'info' uint32 (the last executed step's word;
        .goal / .died), each [count].
        children=None: nothing is kept - a pure evaluation (the leaf simulation of a tree search).  Otherwise slot[children[j]] := the row as
        the last executed step leaves it, as expand() defines a child (for a stopped pair: the state the episode ended in; the episode
        counter is the parent's) - a macro-action of T steps applied to a node.  children: a list / tensor of distinct slots of this
        snapshot; where source and destination are one buffer they must be disjoint from the parents.
        parents, source and from_envs mean what they mean in expand(): slots of `source` (default: this snapshot) or, with from_envs=True,
        the env's current states; parents may repeat, None means 0 .. count-1.
        plans: an integer array [count, T] in host memory - validated here (an id outside the action list raises the ValueError step() raises
        and nothing launches) and uploaded step-major; or a contiguous torch int32 tensor [T, count] on the env's device, used in place and
        unvalidated (an id outside the list is a no-op step of reward 0 that counts in 'length' and raises the sticky F_INVALID_ACTION while
        the pair still runs).  Index tensors on the device are used in place too: an index out of range skips that pair (F_BAD_INDEX, its
        reports stay 0).  Nothing is committed: no env, no mask, no lookahead table, no prepared episode and no slot but the children
        changes, and the number of pairs is not bound by num_envs.  One kernel launch.
        device=True: the results as torch tensors on the env's device ('info' int32), ordered behind the launch on torch's current stream -
        no copy, no host wait; otherwise numpy arrays after one sync.
        limits: None, or one step limit per pair - a list / numpy array of integers in [0, T] (checked here), or a torch int32 tensor on the
        env's device used in place (clamped to [0, T]): pair j executes at most limits[j] steps.  A pair cut by its limit is not 'ended', its
        'info' is its last executed step's; limit 0 reports zeros and leaves the child a copy of the parent.
        path_keys=True: a RolloutPath, whose 'keys' [T, count] hold the key under `fields` (state_keys; what keys() returns for the child
        the pair would leave had it stopped there) of the state after every executed step and 0 for the others - uint64, or an int64 tensor
        with device=True.  Flattened it is what KeyTable.insert takes; fresh_steps() maps `fresh` back to (t, j), and a rollout of the same
        plans with limits = t + 1 materialises that state.  Maps the path form cannot hold raise MapsTooLarge.
        rewards=True / observe='lidar': a RolloutTraj - the fields above ('keys' None without path_keys), 'rewards' int32 [T, count] (the reward
        of step t of pair j, 0 for a step it did not execute; rewards.sum(0) == ret) and 'obs' [T + 1, count, row]: LidarInFront rows in the
        env's configured format, as lidar_observation() returns them (the packed format: the pair (beams, inventory)) - obs[0] the parents,
        obs[t + 1] the state step t leaves, before any reset (the last row of an ended pair is the state its episode ended in), all-zero rows
        for steps not executed.  (obs[t], plans[j, t], rewards[t], obs[t + 1]) is a transition for t < length[j]; transitions() lists them.
        Still one kernel launch and no row leaves the chip's local memory; the rows take (T + 1) * count (rounded up to 64) * row bytes of
        device memory - 65 536 pairs of 64 steps with 80-byte rows are 340 MB - and only what is asked for is allocated.  observe needs
        env.lidar_configure (ValueError otherwise); maps its layout cannot hold raise MapsTooLarge while rewards=True alone keeps the path
        form's limit.  A parent index out of range gives zeros in both fields, obs[0] included.  masks=True is a playout's keyword: ValueError.
        observe='agent_view' (with view_size=V, 1 .. 16, default 5): 'obs' is the AgentMap observation instead, the dict agent_view() returns with the
        same block rule - 'agent_map' int8 [T + 1, count, W, W] (W = 2 * V + 1, the window around the agent, unrotated, 0 outside the map),
        'agent_facing_id' int32 [T + 1, count], 'inventory_items_quantity' int32 [T + 1, count, K]; all three all-zero for steps not executed.  It
        needs no lidar, runs under the path form's layout and keeps its map-size limit; (T + 1) * count (rounded up to 64) * (W * W + 4 + 4 * K)
        bytes of device memory.  view_size without observe='agent_view' is a ValueError unless it is the default."""
        import torch
        env = self.env
        if masks:
            raise ValueError("masks=True: a rollout makes no choice, so there is no mask word to record (playout() records them)")
        check_observe(env, observe, view_size)
        src, n_parents, same_buffer = self._source(source, from_envs, 'rollout')
        dev = torch.device('cuda:%d' % env.device)
        if isinstance(plans, torch.Tensor):
            if plans.dtype != torch.int32 or plans.dim() != 2 or not plans.is_contiguous() or plans.device != dev or plans.shape[0] < 1:
                raise ValueError("plans: a contiguous int32 tensor [T, count] on %s expected" % dev)
            steps, n_plans, a = int(plans.shape[0]), int(plans.shape[1]), plans
        else:
            a = check_plan_ids(plans, env.n_actions)
            n_plans, steps = int(a.shape[0]), int(a.shape[1])
            a = np.ascontiguousarray(a.T)       # step-major [T, count]: 64 lanes read consecutive addresses
        p, c, count = check_rollout(parents, n_plans, children, n_parents, self.capacity, same_buffer, lambda x: tensor_len(dev, 'rollout', x))
        return pairs_call(env, self, 'rollout', src, None if c is None else self._s, p, c, count, steps, device, plans=a, limits=limits, path_keys=path_keys,
                          fields=fields, rewards=rewards, observe=observe, view_size=view_size)

    def playout(self, parents, steps, seed, children=None, from_envs=False, source=None, first_pair=0, record=False, device=False, weights=None,
                limits=None, path_keys=False, fields=KEY_STATE, rewards=False, masks=False, observe=None, view_size=5, table=None, table_weights=None,
                outside='default'):
        """Pair j: the state of parent parents[j] stepped on a private copy up to `steps` times by rollout()'s rules, with a random policy in
        the place of a plan: at every step the action is drawn uniformly among the actions that would succeed from the state the pair is in
        (every action where none would) - the default-policy simulation of a tree search's leaf, in one kernel launch.  The draw is the
        public contract of include/ngw.h, which playout.choose_actions() computes on the host: it depends on (seed, first_pair + j, the step)
        and the state only, so the same parent repeated gives differing playouts, and a call split in two with first_pair set gives the
        rows of the whole one.  Returns a Playout of 'ret', 'length', 'ended', 'info' as rollout() reports them, 'first_action' int32 (the
        action of step 0), each [count], and 'actions': with record=True int32 [steps, count], the action of every executed step (-1 for a
        step the pair did not execute) - as a device tensor it is what rollout() takes as plans, so a playout can be replayed -, else None.
        parents, children, source, from_envs and device mean what they mean in rollout(): children=None keeps nothing, otherwise
        slot[children[j]] := the row as the last executed step leaves it.  Index tensors on the device are used in place: an index out of
        range skips that pair (F_BAD_INDEX; its reports are 0, its actions -1).  Nothing is committed: no env, no mask, no lookahead table,
        no prepared episode and no slot but the children changes.
        weights: None, or float32 [A] - a list / numpy array, or a torch tensor on the env's device used in place: a "heavy" playout.  Every
        step's action is then drawn with probability proportional to the weights among the valid actions (uniformly among them where none
        of them has a weight): rules 3 - 6 of ngw_sample_actions on the playout's own mask word and Philox word, which
        sample.choose_weighted(..., words=playout.playout_words(...)) computes on the host.  A bad weight raises F_BAD_WEIGHT.
        limits, path_keys, fields: as in rollout().  The draws depend on (seed, pair, step) and the state only, so a limited playout is the
        prefix of the unlimited one, and the recorded actions beyond the limit are -1.  With path_keys=True a PlayoutPath: the Playout
        fields and 'keys' [steps, count].
        rewards=True / masks=True / observe='lidar': a PlayoutTraj - the fields above ('keys' None without path_keys), 'rewards' and 'obs' as
        rollout() defines them, and 'masks' uint64 [steps, count] (a torch int64 tensor over the same bits): the valid-action word the choice
        of step t was made under, after the "no action would succeed -> every action" replacement, 0 for a step not executed - so
        playout.choose_actions(masks[t], seed, first_pair + arange(count), t, A) is actions[t], and sample.choose_weighted does the same for a
        weighted playout: what a learner stores to recompute masked log-probabilities.  The memory, the refusals and the zero rows are
        rollout()'s, and so is observe='agent_view' with view_size.
        table=KeyTable, table_weights=[table.buckets, A]: a GUIDED playout - a policy that depends on the state, applied inside the launch.  At
        every step the pair's current state (its key under `fields`: what keys() returns for it; the parent's at step 0, keys[t - 1] later) is
        looked up in `table`; where the table holds it (bucket b = table.lookup(key)) the step's weights are row b of table_weights, otherwise
        they are `weights` (the uniform rule without them) - or, with outside='stop', the pair stops there as if limits[j] were t: not 'ended',
        a kept child receives the state it is in (the leaf of a tree descent).  The choice is the weighted rule on the playout's own mask and
        Philox word; a zero-mass row falls back to the uniform rule, and a bad weight raises F_BAD_WEIGHT only from a row a pair actually read.
        table_weights: a contiguous float32 torch tensor [table.buckets, A] on the env's device, used in place (complete on torch's current
        stream before the call, unchanged until the env's stream has passed it), or a host array of that shape, uploaded (buckets * A * 4 bytes
        per call).  Returns a PlayoutGuided: the PlayoutTraj fields (the per-step ones None unless asked for), 'where' int32 [steps, count] -
        the bucket of every executed step, -1 for a miss and for a step not executed - and 'depth' int32 [count], the leading in-table steps.
        playout.tree_steps(result) lists (bucket, action, t, j) of the in-table steps for the backup, and with path_keys=True the new leaves'
        keys go straight to table.insert.  With an empty table the call is bit-identical to the call without one; with every row equal to
        `weights`, to the weighted playout.  The table is only read; an insert concurrent with the call is not supported.  One kernel launch.
        Refused before a handle is touched: a table of another env, a closed table, table_weights without table (and the reverse), a wrong shape,
        dtype or device, an unknown `outside`, fields == 0.  The running key needs the inventory shadows: the map limit is the keyed call's."""
        import torch
        from .playout import check_guide
        env = self.env
        check_observe(env, observe, view_size)
        guide = check_guide(env, table, table_weights, outside, fields)
        src, n_parents, same_buffer = self._source(source, from_envs, 'playout')
        dev = torch.device('cuda:%d' % env.device)
        p, c, count, steps = check_playout(parents, steps, children, n_parents, self.capacity, same_buffer, lambda x: tensor_len(dev, 'playout', x))
        return pairs_call(env, self, 'playout', src, None if c is None else self._s, p, c, count, steps, device, seed=seed, first_pair=first_pair, record=record,
                          weights=weights, limits=limits, path_keys=path_keys, fields=fields, rewards=rewards, masks=masks, observe=observe,
                          view_size=view_size, table=table, table_weights=table_weights, guide=guide)

    # ------------------------------------------------------------------ slot observations (include/ngw.h ngw_snapshot_lidar / _agent_view / _action_mask)
    def _slots_arg(self, slots):
        """`slots` of a slot observation, checked and uploaded -> what index_arg returns."""
        self._open()
        return index_arg(self.env, slots, self.capacity, 'slots')

    def _enqueue(self, call, count, uploaded, device):
        """One slot observation's launch, ordered as expand() orders its own (enqueue_ordered); this snapshot keeps the uploaded list."""
        enqueue_ordered(self.env, self, call, count, uploaded, device)

    def lidar_observation(self, slots=None, device=False):
        """The LidarInFront observation of saved slots, as env.lidar_observation() returns it for envs: [count, L] in the configured dtype, or the
        pair (beams uint8 [count, B * NC], inventory int16 [count, NI]) with the packed format.  Row j is slot slots[j] (None: every slot),
        bit-identical to what an env holding that state would observe.  Nothing is committed: no env is touched, the env's own lidar rows
        included.  One kernel launch (always the march over maps staged in LDS, whichever form the env's fused path uses).
        slots: None, a list / numpy array (checked here; slots may repeat and their number is not bound by the capacity), or a contiguous torch
        int32 tensor on the env's device, used in place and unchecked: an index out of range gives an all-zero row and raises the sticky
        F_BAD_INDEX (error_flags()).  device=True: torch tensors on the env's device, ordered behind the launch on torch's current stream - no
        copy, no host wait; otherwise numpy arrays after one sync."""
        import torch
        env = self.env
        self._open()
        if env.lidar is None:
            raise ValueError("lidar_observation before env.lidar_configure")
        ptr, count, dev, uploaded = self._slots_arg(slots)
        pad = (count + 63) // 64 * 64           # the wave stores whole 64-row tiles
        if env.lidar_packed:
            rows = torch.empty((pad, env.lidar_row_bytes), dtype=torch.uint8, device=dev)
        else:
            rows = torch.empty((pad, env.lidar_len), dtype=torch.int32 if env.lidar_dtype == np.dtype(np.int32) else torch.int16, device=dev)
        self._enqueue(lambda: _cabi.lib().ngw_snapshot_lidar(env._h, self._s, ptr, count, C.c_void_p(rows.data_ptr())), count, uploaded, device)
        rows = rows[:count]
        if not device:
            rows = rows.cpu().numpy()
        return env._lidar_split(rows) if env.lidar_packed else rows

    def agent_view(self, slots=None, view_size=5, device=False):
        """The AgentMap observation of saved slots: {'agent_map': int8 [count, W, W] with W = 2 * view_size + 1 (the map around each slot's agent,
        0 outside the map), 'agent_facing_id': int32 [count], 'inventory_items_quantity': int32 [count, K]}, gathered in one kernel launch.
        Nothing is committed.  slots and device: as in lidar_observation (an index out of range: an all-zero row, F_BAD_INDEX)."""
        import torch
        env = self.env
        V = int(view_size)
        W = 2 * V + 1
        if not 1 <= V <= 127:
            raise ValueError("view_size must be in 1..127")
        ptr, count, dev, uploaded = self._slots_arg(slots)
        flat = torch.empty((count * W * W + 3) // 4 * 4, dtype=torch.int8, device=dev)      # (the gather stores whole dwords)
        facing = torch.empty(count, dtype=torch.int32, device=dev)
        inv = torch.empty((count, env.n_items), dtype=torch.int32, device=dev)
        self._enqueue(lambda: _cabi.lib().ngw_snapshot_agent_view(env._h, self._s, ptr, count, V, C.c_void_p(flat.data_ptr()), C.c_void_p(facing.data_ptr()),
                                                                  C.c_void_p(inv.data_ptr())), count, uploaded, device)
        view = flat[:count * W * W].view(count, W, W)
        if not device:
            view, facing, inv = view.cpu().numpy(), facing.cpu().numpy(), inv.cpu().numpy()
        return {'agent_map': view, 'agent_facing_id': facing, 'inventory_items_quantity': inv}

    def action_masks(self, slots=None, device=False):
        """The valid-action masks of saved slots: bool [count, n_actions], True where step(a) from slot slots[j]'s state would report
        info['result'] == True under every novelty and wrapper - env.action_masks()'s predicate, fed from the saved row.  Nothing is
        committed: the env's own mask buffer is not touched and stays as current as it was.  One kernel launch.  slots and device: as in
        lidar_observation (an index out of range: an all-False row, F_BAD_INDEX)."""
        import torch
        from .vec_env import unpack_action_masks, unpack_action_masks_device
        env = self.env
        ptr, count, dev, uploaded = self._slots_arg(slots)
        words = torch.empty(count, dtype=torch.int64, device=dev)
        self._enqueue(lambda: _cabi.lib().ngw_snapshot_action_mask(env._h, self._s, ptr, count, C.c_void_p(words.data_ptr())), count, uploaded, device)
        if device:
            return unpack_action_masks_device(words, env.n_actions)
        return unpack_action_masks(words.cpu().numpy().view(np.uint64), env.n_actions)

    def sample_actions(self, slots, weights, seed, first_pair=0, t=0, device=False):
        """VecNovelGridworld.sample_actions over saved slots: one action per entry of `slots`, drawn with probability proportional to
        weights among the actions that slot's state accepts - the prior-guided expansion step of a tree search over a node pool.  slots as
        in lidar_observation (they may repeat, and their number is not bound by the capacity; None: every slot); weights a host array
        [count, A] or a torch float32 tensor [A, count] on the env's device, used in place.  Entry j is pair first_pair + j of the stream of
        `seed` at step number t (the contract of include/ngw.h; sample.choose_weighted on the host), so the same slot repeated gives
        independent draws and a call split in two with first_pair set gives the rows of the whole one.  Returns Sampled(action, mass,
        mask_words), each [count]; an index out of range in a device list: action -1, mass 0, word 0, F_BAD_INDEX.  One kernel launch at
        every map size; nothing is committed."""
        from .sample import sample_call
        self._open()
        return sample_call(self.env, self, self._s, slots, self.capacity, 'slots', weights, seed, first_pair, t, device)

    # ------------------------------------------------------------------ state keys (include/ngw.h ngw_state_keys; state_keys.py)
    def keys(self, slots=None, fields=KEY_STATE, device=False):
        """The 64-bit state keys of saved slots: numpy uint64 [count], entry j the key of slot slots[j] (None: every slot) under the field
        selection `fields` (KEY_* bits; KEY_STATE = map | pose | inventory | selected item) - the public contract of include/ngw.h, which
        state_keys.keys_of_rows() computes on the host for the same state.  Two slots have equal keys exactly when the selected fields are
        equal (up to 64-bit collisions), whichever slot, snapshot, env or rank holds them.  One kernel launch, no LDS staging: it works at
        every map size.  Nothing is committed.
        slots and device: as in lidar_observation (an index out of range in a device list: key 0, F_BAD_INDEX).  device=True: a torch int64
        tensor [count] over the same bits (the convention of action_mask_words), ordered behind the launch on torch's current stream."""
        import torch
        env = self.env
        f = check_fields(fields)
        ptr, count, dev, uploaded = self._slots_arg(slots)
        words = torch.empty(count, dtype=torch.int64, device=dev)
        self._enqueue(lambda: _cabi.lib().ngw_state_keys(env._h, self._s, ptr, count, f, C.c_void_p(words.data_ptr())), count, uploaded, device)
        return words if device else words.cpu().numpy().view(np.uint64)

    def unique(self, slots=None, fields=KEY_STATE, device=False):
        """The groups of equal states among saved slots: (first, inverse), both int64 - inverse[j] is the group of position j of `slots`,
        first[g] the smallest position in group g (positions index `slots`, not the pool; with slots=None they are the slots).  Built from
        keys(): np.unique on the host, or with device=True torch.unique and a scatter-amin on the env's device (no new kernel).  The groups
        are numbered in the order of their keys, which differs between the two (torch compares the keys as int64)."""
        return unique_of_keys(self.keys(slots, fields, device))

    def insert_keys(self, table, slots=None, fields=KEY_STATE, device=False):
        """keys(slots, fields) offered to `table` (a KeyTable of the same env): (keys, KeyInsert(where, fresh)) - which of these slots hold a
        state the table has not seen before.  The keys stay on the device between the two calls: no host wait in between.  device=True: all
        three as torch tensors, ordered behind the launches on torch's current stream; otherwise numpy arrays (keys uint64)."""
        table._open_for(self.env)
        keys = self.keys(slots, fields, device=True)
        found = table.insert(keys, device=device)
        return (keys if device else keys.cpu().numpy().view(np.uint64)), found

    def insert_keys_min(self, table, slots, values, tags=None, fields=KEY_STATE, device=False):
        """keys(slots, fields) offered to `table` (a KeyTable of the same env made with values=True) with one value - and one tag - per slot:
        (keys, KeyBest(where, fresh, best)) - best[j]: slot slots[j] holds its state at a smaller value than the table knew (KeyTable.insert_min).
        values, tags: as there.  The keys stay on the device between the two calls: no host wait in between.  device: as in insert_keys()."""
        table._open_for(self.env)
        keys = self.keys(slots, fields, device=True)
        found = table.insert_min(keys, values, tags, device=device)
        return (keys if device else keys.cpu().numpy().view(np.uint64)), found

    # ------------------------------------------------------------------ successor keys (include/ngw.h ngw_successor_keys)
    def successor_keys(self, slots=None, fields=KEY_STATE, device=False, reports=True):
        """The key of every action's child of saved slots, with no child stored: a SuccessorKeys whose fields are [count, A] - keys[j, a] is
        exactly keys(fields) of the child expand() would write for parent slots[j] (None: every slot) and action a, and reward / done /
        result / info [j, a] exactly what that expand would report (under the env's autoreset setting and horizon; .goal / .died as on an
        Expansion).  reports=False: keys only, the report fields are None.  keys.reshape(-1) is in the pair numbering of expand_all (parent j,
        action a at j * A + a) and goes into KeyTable.insert as it is; insert_successor_keys() does both.  One kernel launch; nothing is
        committed.  Maps up to 34 x 34 (two sets of a wavefront's rows in LDS); beyond that the call raises and expand() + keys() remain.
        slots and device: as in keys() (an index out of range in a device list: a row of zeros in every field, F_BAD_INDEX)."""
        self._open()
        return successor_keys_call(self.env, self, self._s, slots, self.capacity, 'slots', fields, device, reports)

    def insert_successor_keys(self, table, slots=None, fields=KEY_STATE, device=False):
        """successor_keys(slots, fields) offered to `table` (a KeyTable of the same env): (SuccessorKeys, KeyInsert(where, fresh)), where and
        fresh shaped [count, A] - fresh[j, a]: the child of (slots[j], a) is a state the table has not seen, and no earlier (parent, action) of
        this call in row-major order leads to it.  fresh_pairs(fresh) gives the (parent position, action) lists an expand() of exactly the new
        states takes.  The keys stay on the device between the two calls: no host wait in between."""
        table._open_for(self.env)
        return insert_successors(self.successor_keys(slots, fields, device=True), table, device)

    # ------------------------------------------------------------------ walk distances and go-to plans (include/ngw.h ngw_snapshot_walk; walk.py)
    def walk_distances(self, slots=None, device=False):
        """How far saved slots' agents are from facing each item: int32 [count, K], entry (j, k) the fewest Forward / Left / Right moves after
        which the agent of slot slots[j] (None: every slot) faces a cell of id k - 0 where it faces one already, -1 where no reachable pose
        does; air and wall are ordinary columns.  The public integer contract of include/ngw.h, which walk.shortest_walk() computes on the host
        for the same state: a breadth-first search over (row, column, facing) of the saved map and pose under the BASE movement rules - the
        map is static, no pickup and no novelty predicate enters, so under addjump, FireWall, fences and crates this is a geometric quantity,
        not a promise about step().  An admissible heuristic for a best-first search over the pool, a shaping potential, a feature vector.
        One kernel launch, one wavefront per row, at every map size up to 64 x 64; nothing is committed.
        slots and device: as in lidar_observation (an index out of range in a device list: a row of -1, F_BAD_INDEX)."""
        from .walk import walk_call
        self._open()
        return walk_call(self.env, self, self._s, slots, self.capacity, 'slots', None, 0, device, want_plans=False)

    def walk_plans(self, slots, items, steps, device=False):
        """The shortest walk of each saved slot's agent to the nearest cell of an item, as a plan: WalkPlans(plans int32 [steps, count], length
        int32 [count], dist int32 [count, K]).  Column j of `plans` holds the first min(length[j], steps) moves - the env's Forward / Left /
        Right ids - that leave the agent of slot slots[j] facing a cell of id items[j], -1 behind them: the layout and padding of
        playout(record=True).actions, so rollout(slots, plans, limits=length.clamp(0, steps), children=c) with the tensors left on the device
        applies the macro-action "go to the nearest X and face it" to every node in one more launch.  length[j] is the true distance, also
        beyond `steps`, and -1 (a column of -1) where no reachable pose faces the item; dist is walk_distances() of the same rows.  Ties are
        pinned by the contract (the goal pose with the smallest (distance, row, column, facing); walking back, the Forward predecessor before
        the Left and the Right one).  items: an int (one id for all rows), a list / numpy array (checked: ValueError for an id outside
        [0, K)) or a torch int32 tensor on the env's device (used in place: a bad id gives a row of -1 and F_BAD_INDEX).  A spec without a
        Forward, a Left or a Right action raises ValueError; walk_distances() still serves it.  slots, device and the rule: as in
        walk_distances().  One kernel launch; nothing is committed."""
        from .walk import walk_call
        self._open()
        return walk_call(self.env, self, self._s, slots, self.capacity, 'slots', items, steps, device)

    # ------------------------------------------------------------------ the recipe heuristic (include/ngw.h ngw_snapshot_recipe_costs; search.py)
    def recipe_costs(self, slots=None, costs=None, scale=1, source=None, from_envs=False, device=False):
        """What saved slots' states still have to pay in crafts, extractions and breaks before they hold the goal item, at the least: int32
        [count], entry j the relaxed-plan cost of slot slots[j] (None: every slot) under search.recipe_program(spec, costs, scale) - costs /
        scale as search() takes them - read off the slot's inventory and, for the tools the program flags (the Pogostick tap), their number
        on its map.  The public integer contract of include/ngw.h, which search.recipe_cost_reference() computes on the host for the same
        state.  The heuristic term of an A* over the pool (search.RecipeHeuristic runs it inside run()), a shaping potential, a progress
        feature; moves are not in it - walk_distances() bounds those.  source / from_envs: the rows of another Snapshot of the same env /
        the env's current states, as in expand().  One kernel launch, no LDS staging: every map size; nothing is committed.
        slots and device: as in keys() (they may repeat; IDX_NONE in a device list: 0; an index out of range there: 0, F_BAD_INDEX)."""
        from .search import recipe_call
        src, n_rows, _ = self._source(source, from_envs, 'recipe_costs')
        return recipe_call(self.env, self, src, slots, n_rows, 'envs' if from_envs else 'slots', costs, scale, device)

    # ------------------------------------------------------------------ device-side frontiers (include/ngw.h ngw_frontier_*; frontier.py)
    def frontier(self, capacity):
        """A Frontier of `capacity` entries for this snapshot: index lists padded with IDX_NONE and a slot cursor on the device, so that
        `fresh` flags become the parents, actions and child slots of the next expand() without the host learning how many there are
        (frontier.py).  Every call that takes a device index list skips a pair whose index is IDX_NONE and raises no F_BAD_INDEX for it."""
        from .frontier import Frontier
        self._open()
        return Frontier(self, capacity)

    # ------------------------------------------------------------------ device-side search runs (include/ngw.h ngw_search_*; search.py)
    def search(self, table, capacity, costs=None, scale=1, keep=None, stop_at_goals=False, open_list=False, heuristic=None, prune=False):
        """A Search over this snapshot - the node pool - and `table` (a KeyTable of the same env made with values=True): whole iterations of
        the label-correcting loop of key_table.py's docstring, `capacity` parents each, enqueued from one call with no host wait in between;
        it keeps the cost and the bucket every slot was reached with and the cheapest goal reached (search.py says what an iteration is).
        costs: None - the step costs times `scale`, rounded - or one int32 per action; keep: None or the k cheapest improved states that go
        on; stop_at_goals: ended states are not expanded.  ValueError for a table without values and for keep > capacity; maps beyond
        successor_keys' 34 x 34 raise what successor_keys raises.  open_list=True (with keep=k): a best-first search over an open list - the k
        open states of the smallest f = g + h of the WHOLE list are expanded per iteration -, heuristic: None, a search.WalkHeuristic or a
        search.RecipeHeuristic, prune: states that cannot beat the goal are closed unexpanded (search.Search says what each does).  Closed by its close() and with
        this snapshot."""
        from .search import Search
        self._open()
        s = Search(self, table, capacity, costs, scale, keep, stop_at_goals, open_list, heuristic, prune)
        self.__dict__.setdefault('_searches', []).append(s)
        return s

    # ------------------------------------------------------------------ device-side tree-search runs (include/ngw.h ngw_tree_*; tree.py)
    def tree_search(self, table, playouts, steps, c=1.0, q_init=0.0, priors=False, weights=None, fields=KEY_STATE, plain_backup=False, spread=1, discount=1.0,
                    rows16=0):
        """A TreeSearch over `table` (a KeyTable of the same env) rooted in this snapshot's slots - or, with start(from_envs=True), in the envs'
        current states -: whole MCTS iterations of `playouts` pairs and `steps` steps each - a guided playout, the new leaves inserted, an
        integer every-visit backup, the PUCT rows recomputed under each node's valid-action mask -, enqueued from one call with no host wait in
        between; it keeps visit counts, return sums and mask words per bucket of the table (tree.py says what an iteration is).  c, q_init: the
        PUCT rule's; priors=True: a [buckets, A] tensor of priors for the caller to fill; weights: the default policy's, None: uniform; fields:
        the KEY_* selection of a node.  spread: 1 to 64, the PUCT choices with virtual visits a row allots (above 1 the pairs of one root diverge
        inside the tree); discount: a float in [0, 1] per executed step, applied in integers (tree.py).  ValueError for a table of another env, playouts * steps or buckets * A beyond 2^31 - 1, fields == 0, a c
        or q_init that is not finite; maps beyond the keyed guided playout's limit raise what playout(table=) raises.  Closed by its close()
        and with this snapshot."""
        from .tree import TreeSearch
        self._open()
        t = TreeSearch(self, table, playouts, steps, c, q_init, priors, weights, fields, plain_backup, spread, discount, rows16)
        self.__dict__.setdefault('_searches', []).append(t)
        return t

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
            for s in list(self.__dict__.get('_searches', ())):
                s.close()
            _cabi.check(_cabi.lib().ngw_snapshot_destroy(self.env._h, self._s))
        self._invalidate()
        snaps = self.env.__dict__.get('_snapshots')
        if snaps and self in snaps:
            snaps.remove(self)

    def _invalidate(self):
        """The handle is gone (or going), and the buffer with it."""
        self._s = C.c_void_p()
        self._keep = None
        for s in self.__dict__.pop('_searches', ()):
            s._invalidate()
