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


def check_action_ids(actions, n_actions, name='actions'):
    """The host-side check of one action id per pair given as a list / numpy array: integer dtype, one dimension, every id in the action
    list (ValueError("<a> is not in list") otherwise, what step() raises).  Returns a contiguous int32 array."""
    if actions is None:
        raise ValueError("%s: one action id per pair expected" % name)
    a = np.asarray(actions)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int32)
    if a.dtype.kind not in 'iu':
        raise ValueError("%s: integer action ids expected, got dtype %s" % (name, a.dtype))
    if a.ndim != 1:
        raise ValueError("%s: a one-dimensional list of action ids expected, got shape %s" % (name, a.shape))
    bad = (a < 0) | (a >= n_actions)
    if bad.any():
        raise ValueError("%d is not in list" % int(a[bad][0]))
    return np.ascontiguousarray(a, np.int32)


def check_expand(parents, actions, children, n_parents, capacity, n_actions, same_buffer, device_len=None):
    """The host-side checks of one expand call: parents index rows [0, n_parents) and may repeat, children index slots [0, capacity) and
    must be distinct, actions are ids of the action list, the three have one length (None = no list: 0 .. count-1, which must exist), and -
    where source and destination are the same buffer - no child is also a parent.  device_len(x): the length of x when it is a device
    tensor to be used in place (its values are then not checked), else None.  Returns (parents, actions, children, count): contiguous
    int32 arrays, None, or the device tensors themselves."""
    on_dev = (lambda x: None) if device_len is None else device_len
    n_p, n_a, n_c = on_dev(parents), on_dev(actions), on_dev(children)
    if n_p is None and parents is not None:
        parents = check_indices(parents, n_parents, False, 'parents')
        n_p = int(parents.size)
    if n_a is None:
        actions = check_action_ids(actions, n_actions)
        n_a = int(actions.size)
    if n_c is None and children is not None:
        children = check_indices(children, capacity, True, 'children')
        n_c = int(children.size)
    count = pair_count(pair_count(n_p, n_a, n_a), n_c, n_a)
    if parents is None and count > n_parents:
        raise ValueError("parents: no list given and %d pairs for %d rows" % (count, n_parents))
    if count > capacity:
        raise ValueError("children: %d pairs for a snapshot of %d slots" % (count, capacity))
    if same_buffer and count and on_dev(parents) is None and on_dev(children) is None:
        hp = np.arange(count) if parents is None else parents
        hc = np.arange(count) if children is None else children
        both = np.intersect1d(hp, hc)
        if both.size:
            raise ValueError("children: slot %d is also a parent of the same call (source and destination are one buffer)" % int(both[0]))
    return parents, actions, children, count


def check_plan_ids(plans, n_actions, name='plans'):
    """The host-side check of one action sequence per pair given as a list / numpy array [count, T]: integer dtype, two dimensions, at
    least one step, every id in the action list (ValueError("<a> is not in list") otherwise, what step() raises).  Returns a contiguous int32
    array [count, T]."""
    if plans is None:
        raise ValueError("%s: one action sequence per pair expected" % name)
    a = np.asarray(plans)
    if a.ndim == 2 and a.shape[0] == 0 and a.shape[1] >= 1:
        return np.zeros(a.shape, np.int32)      # (an empty list has no dtype of its own)
    if a.dtype.kind not in 'iu':
        raise ValueError("%s: integer action ids expected, got dtype %s" % (name, a.dtype))
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("%s: action ids shaped [count, T] with T >= 1 expected, got shape %s" % (name, a.shape))
    bad = (a < 0) | (a >= n_actions)
    if bad.any():
        raise ValueError("%d is not in list" % int(a[bad][0]))
    return np.ascontiguousarray(a, np.int32)


def check_rollout(parents, n_plans, children, n_parents, capacity, same_buffer, device_len=None):
    """The host-side checks of one rollout call's index lists: parents index rows [0, n_parents) and may repeat (None = 0 .. count-1, which
    must exist); children - None: nothing is kept - index slots [0, capacity) and must be distinct; both have the plans' length n_plans,
    and - where source and destination are the same buffer - no child is also a parent.  device_len(x): the length of x when it is a
    device tensor to be used in place (its values are then not checked), else None.  Returns (parents, children, count): contiguous int32
    arrays, None, or the device tensors themselves."""
    on_dev = (lambda x: None) if device_len is None else device_len
    n_p, n_c = on_dev(parents), on_dev(children)
    if n_p is None and parents is not None:
        parents = check_indices(parents, n_parents, False, 'parents')
        n_p = int(parents.size)
    if n_c is None and children is not None:
        children = check_indices(children, capacity, True, 'children')
        n_c = int(children.size)
    count = pair_count(pair_count(n_p, n_plans, n_plans), n_c, n_plans)
    if parents is None and count > n_parents:
        raise ValueError("parents: no list given and %d pairs for %d rows" % (count, n_parents))
    if children is not None and count > capacity:
        raise ValueError("children: %d pairs for a snapshot of %d slots" % (count, capacity))
    if same_buffer and count and children is not None and on_dev(parents) is None and on_dev(children) is None:
        hp = np.arange(count) if parents is None else parents
        both = np.intersect1d(hp, children)
        if both.size:
            raise ValueError("children: slot %d is also a parent of the same call (source and destination are one buffer)" % int(both[0]))
    return parents, children, count


def check_slots(slots, capacity, device_len=None):
    """The host-side checks of the slot list of one slot observation (lidar_observation / agent_view / action_masks of a Snapshot): None = every
    slot, 0 .. capacity-1; a list / numpy array indexes slots [0, capacity) and may repeat (its length is not bound by the capacity).
    device_len(x): the length of x when it is a device tensor to be used in place (its values are then not checked), else None.  Returns
    (slots, count): a contiguous int32 array, None, or the device tensor itself."""
    if slots is None:
        return None, int(capacity)
    n = None if device_len is None else device_len(slots)
    if n is not None:
        return slots, int(n)
    slots = check_indices(slots, capacity, False, 'slots')
    return slots, int(slots.size)


def index_arg(env, idx, limit, name):
    """One index list of a call that reads rows by index (the slot observations, the state keys), checked and uploaded: None, a list / numpy
    array (check_slots) or a contiguous torch int32 tensor on the env's device, used in place.  -> (device pointer or None, count, torch
    device, the uploaded tensor or None)."""
    import torch
    dev = torch.device('cuda:%d' % env.device)

    def device_len(x):
        if not isinstance(x, torch.Tensor):
            return None
        if x.dtype != torch.int32 or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
            raise ValueError("%s: a contiguous one-dimensional int32 tensor on %s expected" % (name, dev))
        return int(x.numel())
    s, count = check_slots(idx, limit, device_len)
    uploaded = None
    if isinstance(s, np.ndarray):
        s = uploaded = torch.from_numpy(s).to(dev)
    return (C.c_void_p(s.data_ptr()) if s is not None and count else None), count, dev, uploaded


def enqueue_ordered(env, holder, call, count, uploaded, device):
    """One launch on the env's stream that reads and writes torch tensors: the env's stream waits for torch's current one (uploads, the
    allocations of the outputs, the caller's own tensors), and behind the launch either torch's stream waits for the env's (device=True: no
    host wait) or the host does.  `holder._keep` keeps an uploaded list alive until the next call of the holder has synchronised."""
    import torch
    if holder._keep:
        env.sync()                              # (the previous call has read its lists: they may be released now)
        holder._keep = None
    if count:
        env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, True)
        _cabi.check(call())
        holder._keep = [uploaded] if uploaded is not None else None
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
        self._open()
        if source is not None and from_envs:
            raise ValueError("expand: give either source or from_envs")
        src = self if source is None else source
        if not from_envs:
            if not isinstance(src, Snapshot):
                raise ValueError("source: a Snapshot expected")
            src._open()
            if src.env is not env:
                raise ValueError("source: a snapshot of another env")
        n_parents = env.num_envs if from_envs else src.capacity
        dev = torch.device('cuda:%d' % env.device)

        def device_len(x):
            if not isinstance(x, torch.Tensor):
                return None
            if x.dtype != torch.int32 or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
                raise ValueError("a contiguous one-dimensional int32 tensor on %s expected" % dev)
            return int(x.numel())
        p, a, c, count = check_expand(parents, actions, children, n_parents, self.capacity, env.n_actions, not from_envs and src is self, device_len)
        ptr, uploaded = [], []
        for x in (p, a, c):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(x).to(dev)
                uploaded.append(x)
            ptr.append(C.c_void_p(x.data_ptr()) if x is not None and count else None)
        reward = torch.zeros(count, dtype=torch.int32, device=dev)
        done = torch.zeros(count, dtype=torch.uint8, device=dev)
        info = torch.zeros(count, dtype=torch.int32, device=dev)
        if self._keep:
            env.sync()                          # (the previous call has read its lists: they may be released now)
            self._keep = None
        if count:
            # uploads, zero fills and the caller's own tensors are work of torch's current stream, the launch runs on the env's: it waits for them
            env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, True)
            _cabi.check(_cabi.lib().ngw_snapshot_expand(env._h, None if from_envs else src._s, ptr[0], ptr[1], self._s, ptr[2], int(count),
                                                        C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()), C.c_void_p(info.data_ptr())))
            self._keep = uploaded or None
        if device:
            if count:
                env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, False)
            return Expansion(reward, done.view(torch.bool), (info & 1).bool(), info)
        env.sync()
        self._keep = None
        words = info.cpu().numpy().view(np.uint32)
        return Expansion(reward.cpu().numpy(), done.cpu().numpy().view(np.bool_), (words & 1).astype(np.bool_), words)

    def expand_all(self, parents, first_child, from_envs=False, source=None, device=False):
        """Every parent with every action id 0 .. A-1 (A = env.n_actions): the child of (parents[p], a) goes to slot first_child + p * A + a.
        Returns the Expansion shaped [len(parents), A]."""
        p, a, c, shape = all_actions_pairs(parents, first_child, self.env.n_actions)
        return self.expand(p, a, c, from_envs=from_envs, source=source, device=device).reshape(*shape)

    def rollout(self, parents, plans, children=None, from_envs=False, source=None, device=False):
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
        no copy, no host wait; otherwise numpy arrays after one sync."""
        import torch
        from .vec_env import PlanEval
        env = self.env
        self._open()
        if source is not None and from_envs:
            raise ValueError("rollout: give either source or from_envs")
        src = self if source is None else source
        if not from_envs:
            if not isinstance(src, Snapshot):
                raise ValueError("source: a Snapshot expected")
            src._open()
            if src.env is not env:
                raise ValueError("source: a snapshot of another env")
        n_parents = env.num_envs if from_envs else src.capacity
        dev = torch.device('cuda:%d' % env.device)

        def device_len(x):
            if not isinstance(x, torch.Tensor):
                return None
            if x.dtype != torch.int32 or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
                raise ValueError("a contiguous one-dimensional int32 tensor on %s expected" % dev)
            return int(x.numel())
        if isinstance(plans, torch.Tensor):
            if plans.dtype != torch.int32 or plans.dim() != 2 or not plans.is_contiguous() or plans.device != dev or plans.shape[0] < 1:
                raise ValueError("plans: a contiguous int32 tensor [T, count] on %s expected" % dev)
            steps, n_plans, a = int(plans.shape[0]), int(plans.shape[1]), plans
        else:
            a = check_plan_ids(plans, env.n_actions)
            n_plans, steps = int(a.shape[0]), int(a.shape[1])
            a = np.ascontiguousarray(a.T)       # step-major [T, count]: 64 lanes read consecutive addresses
        p, c, count = check_rollout(parents, n_plans, children, n_parents, self.capacity, not from_envs and src is self, device_len)
        ptr, uploaded = [], []
        for x in (p, a, c):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(x).to(dev)
                uploaded.append(x)
            ptr.append(C.c_void_p(x.data_ptr()) if x is not None and count else None)
        ret = torch.zeros(count, dtype=torch.int32, device=dev)
        length = torch.zeros(count, dtype=torch.int32, device=dev)
        ended = torch.zeros(count, dtype=torch.uint8, device=dev)
        info = torch.zeros(count, dtype=torch.int32, device=dev)
        if self._keep:
            env.sync()                          # (the previous call has read its lists: they may be released now)
            self._keep = None
        if count:
            # uploads, zero fills and the caller's own tensors are work of torch's current stream, the launch runs on the env's: it waits for them
            env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, True)
            _cabi.check(_cabi.lib().ngw_snapshot_rollout(env._h, None if from_envs else src._s, ptr[0], ptr[1], int(count), steps,
                                                         None if c is None else self._s, ptr[2], int(count), C.c_void_p(ret.data_ptr()),
                                                         C.c_void_p(length.data_ptr()), C.c_void_p(ended.data_ptr()), C.c_void_p(info.data_ptr())))
            self._keep = uploaded or None
        if device:
            if count:
                env.stream_order(torch.cuda.current_stream(env.device).cuda_stream, False)
            return PlanEval(ret, length, ended.view(torch.bool), info)
        env.sync()
        self._keep = None
        return PlanEval(ret.cpu().numpy(), length.cpu().numpy(), ended.cpu().numpy().view(np.bool_), info.cpu().numpy().view(np.uint32))

    # ------------------------------------------------------------------ slot observations (include/ngw.h ngw_snapshot_lidar / _agent_view / _action_mask)
    def _slots_arg(self, slots):
        """`slots` of a slot observation, checked and uploaded -> (device pointer or None, count, torch device, the uploaded tensor or None)."""
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
        from .vec_env import unpack_action_masks
        env = self.env
        ptr, count, dev, uploaded = self._slots_arg(slots)
        words = torch.empty(count, dtype=torch.int64, device=dev)
        self._enqueue(lambda: _cabi.lib().ngw_snapshot_action_mask(env._h, self._s, ptr, count, C.c_void_p(words.data_ptr())), count, uploaded, device)
        if device:
            bits = torch.arange(env.n_actions, device=words.device, dtype=torch.int64)
            return ((words[:, None] >> bits) & 1).bool()
        return unpack_action_masks(words.cpu().numpy().view(np.uint64), env.n_actions)

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
