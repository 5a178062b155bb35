"""Walk distances and go-to plans: the contract of include/ngw.h (ngw_snapshot_walk) on the host in numpy, and the one launch behind
Snapshot.walk_distances / walk_plans and VecNovelGridworld.walk_distances / walk_plans.

    facing NORTH 0, SOUTH 1, WEST 2, EAST 3;  dr = (-1, 1, 0, 0), dc = (0, 0, -1, 1);  left = (2, 3, 1, 0), right = (3, 2, 0, 1)
    Forward (r, c, f) -> (r + dr[f], c + dc[f], f) iff that cell is inside the map and holds id 0;  Left / Right turn in place;  every move costs 1

D(p) is the breadth-first distance of pose p from the agent's pose, dist[k] the smallest D over the reachable poses whose front cell holds id k
(-1: none), the goal pose the one that minimises (D, r, c, f), and the path the walk back from it that prefers the Forward predecessor, then the
Left one, then the Right one.  The map is static - no pickup, no novelty predicate - so under a Jump action or a FireWall / fence / crate
predicate this is a geometric quantity, not a promise about what step() does.  The device computes the same numbers without the copy."""
import collections

import numpy as np

from .spec import ACT_RIGHT

DR, DC = (-1, 1, 0, 0), (0, 0, -1, 1)
LEFT, RIGHT = (2, 3, 1, 0), (3, 2, 0, 1)
_NONE = np.uint32(0xFFFFFFFF)


class WalkPlans(collections.namedtuple('WalkPlans', 'plans length dist')):
    """What walk_plans() returns: 'plans' int32 [T, count] - column j the first min(length, T) moves of the shortest walk of row j to its item, -1
    behind them (the layout and padding of playout(record=True).actions: what rollout() takes as device plans) -, 'length' int32 [count] - the
    true number of moves, -1 where no reachable pose faces the item -, 'dist' int32 [count, K] - walk_distances() of the same rows.  numpy arrays,
    or torch tensors on the env's device."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)


def walk_action_ids(spec):
    """(forward, left, right): the lowest action id of each of the three kinds in `spec` (an EnvSpec or its compiled NgwSpec) - the ids a plan is
    written in -, None for a kind the action table lacks."""
    c = spec.compile() if hasattr(spec, 'compile') else spec
    ids = [None, None, None]
    for a in range(c.n_actions - 1, -1, -1):
        if c.act_kind[a] <= ACT_RIGHT:
            ids[c.act_kind[a]] = a
    return tuple(ids)


def plan_action_ids(spec):
    """walk_action_ids(spec), or ValueError naming the kind a plan cannot be written without."""
    ids = walk_action_ids(spec)
    for name, a in zip(('Forward', 'Left', 'Right'), ids):
        if a is None:
            raise ValueError("walk plans need a Forward, a Left and a Right action; this spec has no %s (the distances are available)" % name)
    return ids


def walk_fields(maps, loc, facing):
    """D of every pose of n states at once: (int32 [n, 4, S, S] indexed [row, f, r, c], -1 where a pose is not reachable; the number of
    breadth-first layers of the deepest row).  maps int8 [n, S*S] or [n, S, S], loc [n, 2], facing [n]."""
    loc, facing = np.asarray(loc).astype(np.int64).reshape(-1, 2), np.asarray(facing).astype(np.int64).reshape(-1)
    n = len(facing)
    m = np.ascontiguousarray(maps, np.int8).reshape(n, -1)
    S = int(round(m.shape[1] ** 0.5))
    if S * S != m.shape[1]:
        raise ValueError("maps: square maps expected, got %d cells a row" % m.shape[1])
    air = m.reshape(n, S, S) == 0
    R = np.zeros((n, 4, S, S), bool)
    ok = (loc >= 0).all(1) & (loc < S).all(1) & (facing >= 0) & (facing < 4)
    at = np.nonzero(ok)[0]
    R[at, facing[at], loc[at, 0], loc[at, 1]] = True
    D = np.where(R, 0, -1).astype(np.int32)
    d = 0
    while True:
        ns, we = R[:, 0] | R[:, 1], R[:, 2] | R[:, 3]
        new = np.empty_like(R)
        new[:, 0], new[:, 1], new[:, 2], new[:, 3] = we, we, ns, ns
        new[:, 0, :-1, :] |= R[:, 0, 1:, :] & air[:, :-1, :]          # NORTH: from the row below into an air cell
        new[:, 1, 1:, :] |= R[:, 1, :-1, :] & air[:, 1:, :]
        new[:, 2, :, :-1] |= R[:, 2, :, 1:] & air[:, :, :-1]
        new[:, 3, :, 1:] |= R[:, 3, :, :-1] & air[:, :, 1:]
        new &= ~R
        if not new.any():
            return D, d
        d += 1
        D[new] = d
        R |= new


def _front_ids(m):
    """The id in front of every pose of maps m [n, S, S]: int16 [n, 4, S, S], -1 where the front cell lies outside the map."""
    n, S = m.shape[0], m.shape[1]
    front = np.full((n, 4, S, S), -1, np.int16)
    front[:, 0, 1:, :], front[:, 1, :-1, :] = m[:, :-1, :], m[:, 1:, :]
    front[:, 2, :, 1:], front[:, 3, :, :-1] = m[:, :, :-1], m[:, :, 1:]
    return front


def walk_goals(maps, D, n_items):
    """uint32 [n, K]: min(D << 16 | r << 10 | c << 4 | f) over the reachable poses that face id k - the distance and the goal pose in one word -,
    0xFFFFFFFF where there is none."""
    n, _, S, _ = D.shape
    front = _front_ids(np.ascontiguousarray(maps, np.int8).reshape(n, S, S))
    f, r, c = np.meshgrid(np.arange(4), np.arange(S), np.arange(S), indexing='ij')
    pose = (r << 10 | c << 4 | f).astype(np.uint32)[None]
    key = np.where(D >= 0, (D.astype(np.uint32) << np.uint32(16)) | pose, _NONE)
    best = np.empty((n, n_items), np.uint32)
    for k in range(n_items):
        best[:, k] = np.where(front == k, key, _NONE).reshape(n, -1).min(1)
    return best


def distances_of_goals(best):
    return np.where(best == _NONE, -1, best >> np.uint32(16)).astype(np.int32)


def walk_back(m, D, goal, ids):
    """The moves from the agent's pose to the pose packed in `goal` (one word of walk_goals), in the ids (forward, left, right): map m [S, S], D
    [4, S, S] of the same row."""
    S = m.shape[0]
    r, c, f = int(goal >> 10) & 63, int(goal >> 4) & 63, int(goal) & 3
    moves = []
    for d in range(int(goal >> 16), 0, -1):
        pr, pc = r - DR[f], c - DC[f]
        if 0 <= pr < S and 0 <= pc < S and m[r, c] == 0 and D[f, pr, pc] == d - 1:
            moves.append(ids[0])
            r, c = pr, pc
        elif D[RIGHT[f], r, c] == d - 1:                              # (the pose that reaches this one by Left)
            moves.append(ids[1])
            f = RIGHT[f]
        else:
            moves.append(ids[2])
            f = LEFT[f]
    return moves[::-1]


class ShortestWalk(collections.namedtuple('ShortestWalk', 'dist field layers goals map ids')):
    """shortest_walk()'s answer for one state: 'dist' int32 [K], 'field' int32 [4, S, S] (D of every pose, -1: not reachable), 'layers' (the
    largest D), and plan(item) -> (the list of action ids of the whole path, its length; ([], -1) where no pose faces the item)."""
    __slots__ = ()

    def plan(self, item):
        if not 0 <= item < len(self.dist):
            raise ValueError("item %d outside [0, %d)" % (item, len(self.dist)))
        if any(a is None for a in self.ids):
            plan_action_ids_missing(self.ids)
        if self.dist[item] < 0:
            return [], -1
        return walk_back(self.map, self.field, self.goals[item], self.ids), int(self.dist[item])


def plan_action_ids_missing(ids):
    name = ('Forward', 'Left', 'Right')[[a is None for a in ids].index(True)]
    raise ValueError("walk plans need a Forward, a Left and a Right action; this spec has no %s (the distances are available)" % name)


def shortest_walk(map, pose, spec):
    """The contract for ONE state on the host: map int8 [S, S] (or [S*S]), pose (r, c, f), spec an EnvSpec (or its compiled NgwSpec: n_items and the
    ids plans are written in).  -> ShortestWalk."""
    c = spec.compile() if hasattr(spec, 'compile') else spec
    m = np.ascontiguousarray(map, np.int8).reshape(1, -1)
    D, layers = walk_fields(m, [[pose[0], pose[1]]], [pose[2]])
    best = walk_goals(m, D, c.n_items)
    S = D.shape[2]
    return ShortestWalk(distances_of_goals(best)[0], D[0], layers, best[0], m.reshape(S, S), walk_action_ids(c))


def shortest_walks(rows, items, steps, spec):
    """The loop the device call replaces, for rows shaped like get_state() / Snapshot.state() ('map', 'loc', 'facing'): -> WalkPlans of numpy arrays
    (items None: plans and length None).  items: one id per row."""
    c = spec.compile() if hasattr(spec, 'compile') else spec
    D, _ = walk_fields(rows['map'], rows['loc'], rows['facing'])
    n, _, S, _ = D.shape
    best = walk_goals(rows['map'], D, c.n_items)
    dist = distances_of_goals(best)
    if items is None:
        return WalkPlans(None, None, dist)
    ids = plan_action_ids(c)
    items, steps = check_items(items, n, c.n_items), check_steps(steps)
    m = np.ascontiguousarray(rows['map'], np.int8).reshape(n, S, S)
    plans, length = np.full((steps, n), -1, np.int32), dist[np.arange(n), items].astype(np.int32)
    for j in np.nonzero(length > 0)[0]:
        moves = walk_back(m[j], D[j], best[j, items[j]], ids)[:steps]
        plans[:len(moves), j] = moves
    return WalkPlans(plans, length, dist)


def check_items(items, count, n_items, device_len=None):
    """The host-side check of walk_plans' `items`: an int (one id for every row), a list / numpy array of `count` integers - each in [0, n_items),
    ValueError otherwise - -> a contiguous int32 array; or - device_len(x) gives its length - a device int32 tensor of `count` elements, used in
    place with its VALUES unchecked (an id out of range gives a row of -1 and raises F_BAD_INDEX)."""
    n = None if device_len is None else device_len(items)
    if n is None:
        if isinstance(items, bool) or items is None:
            raise ValueError("items: an item id, or one per row, expected, got %r" % (items,))
        a = np.asarray(items)
        if a.ndim == 0:
            a = np.full(count, a)
        if a.ndim != 1 or (a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer))):
            raise ValueError("items: a one-dimensional list of integer item ids expected")
        if a.size and (a.min() < 0 or a.max() >= n_items):
            raise ValueError("items: %d outside [0, %d)" % (int(a[(a < 0) | (a >= n_items)][0]), n_items))
        items, n = np.ascontiguousarray(a, dtype=np.int32), int(a.size)
    if n != count:
        raise ValueError("items: %d items for %d rows" % (n, count))
    return items


def check_steps(steps):
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
        raise ValueError("steps: an integer number of steps expected, got %r" % (steps,))
    if steps < 1:
        raise ValueError("steps: at least one step expected, got %d" % steps)
    return int(steps)


def walk_call(env, holder, s, idx, limit, name, items, steps, device, want_plans=True):
    """The one launch behind Snapshot.walk_distances / walk_plans (s: the snapshot's C handle) and VecNovelGridworld's (s None: the envs' current
    states): idx indexes rows [0, limit); want_plans=False asks for the distances alone (items and steps are then not read); `holder` keeps
    uploaded lists alive.  -> the distances, or a WalkPlans."""
    import ctypes as C

    import torch

    from . import _cabi
    from .snapshot import check_slots, enqueue_ordered, tensor_len, upload
    K = env.n_items
    dev = torch.device('cuda:%d' % env.device)
    if not want_plans:
        items = None
    else:
        if items is None:
            raise ValueError("items: an item id, or one per row, expected, got None")
        steps = check_steps(steps)
        plan_action_ids(env.cspec)
    rows, count = check_slots(idx, limit, lambda x: tensor_len(dev, name, x), False, name)
    if items is not None:
        items = check_items(items, count, K, lambda x: tensor_len(dev, 'items', x))
    (ptr, iptr), uploaded = upload(dev, count, rows, items)
    dist = torch.empty((count, K), dtype=torch.int32, device=dev)
    plans = length = None
    if items is not None:
        plans = torch.empty((steps, count), dtype=torch.int32, device=dev)
        length = torch.empty(count, dtype=torch.int32, device=dev)
    p = [None if x is None else C.c_void_p(x.data_ptr()) for x in (dist, plans, length)]
    enqueue_ordered(env, holder, lambda: _cabi.lib().ngw_snapshot_walk(env._h, s, ptr, count, iptr, steps if items is not None else 0, *p), count, uploaded,
                    device)
    if items is None:
        return dist if device else dist.cpu().numpy()
    return WalkPlans(plans, length, dist) if device else WalkPlans(plans.cpu().numpy(), length.cpu().numpy(), dist.cpu().numpy())
