"""The walk contract of include/ngw.h (ngw_snapshot_walk) restated with plain Python: one pose at a time through a queue, written from the contract
text and not from gym_novel_gridworlds_amd/walk.py (whose layered boolean planes the tests hold to this).

    facing NORTH 0, SOUTH 1, WEST 2, EAST 3;  Forward enters the cell in front iff it is inside the map and holds id 0;  Left / Right turn in place"""
from collections import deque

import numpy as np

DR, DC = (-1, 1, 0, 0), (0, 0, -1, 1)
LEFT, RIGHT = (2, 3, 1, 0), (3, 2, 0, 1)


def moves_from(m, S, p):
    """The poses one move away from p = (r, c, f), in the order Forward, Left, Right (a blocked Forward is left out)."""
    r, c, f = p
    out = []
    fr, fc = r + DR[f], c + DC[f]
    if 0 <= fr < S and 0 <= fc < S and m[fr][fc] == 0:
        out.append((fr, fc, f))
    out.append((r, c, LEFT[f]))
    out.append((r, c, RIGHT[f]))
    return out


def distances(m, pose):
    """{pose: D} of every reachable pose of map m (S lists of S ids) from `pose`."""
    S = len(m)
    D = {tuple(pose): 0}
    queue = deque([tuple(pose)])
    while queue:
        p = queue.popleft()
        for q in moves_from(m, S, p):
            if q not in D:
                D[q] = D[p] + 1
                queue.append(q)
    return D


def front(m, S, p):
    r, c, f = p
    fr, fc = r + DR[f], c + DC[f]
    return m[fr][fc] if 0 <= fr < S and 0 <= fc < S else None


def goals(m, D, K):
    """[the goal pose of item k, or None] for k < K: the reachable pose facing k with the smallest (D, r, c, f)."""
    S = len(m)
    best = [None] * K
    for p, d in D.items():
        k = front(m, S, p)
        if k is not None and 0 <= k < K and (best[k] is None or (d,) + p < best[k]):
            best[k] = (d,) + p
    return [None if b is None else b[1:] for b in best]


def path(m, D, goal, ids):
    """The plan to `goal` in the ids (forward, left, right): the walk back that takes the Forward predecessor first, then the pose that reaches the
    current one by Left, then the one that reaches it by Right."""
    S = len(m)
    q, moves = tuple(goal), []
    while D[q] > 0:
        r, c, f = q
        d = D[q]
        fwd = (r - DR[f], c - DC[f], f)
        by_left = (r, c, LEFT.index(f))          # left[g] == f
        by_right = (r, c, RIGHT.index(f))
        if 0 <= fwd[0] < S and 0 <= fwd[1] < S and m[r][c] == 0 and D.get(fwd) == d - 1:
            moves.append(ids[0]); q = fwd
        elif D.get(by_left) == d - 1:
            moves.append(ids[1]); q = by_left
        else:
            assert D.get(by_right) == d - 1, (q, d)
            moves.append(ids[2]); q = by_right
    return moves[::-1]


def search(map_row, loc, facing, K):
    """One state searched: (the map as lists, {pose: D}, the goal poses, dist [K]).  map_row: S*S ids."""
    cells = [int(v) for v in np.asarray(map_row).reshape(-1)]
    S = int(round(len(cells) ** 0.5))
    m = [cells[r * S:(r + 1) * S] for r in range(S)]
    D = distances(m, (int(loc[0]), int(loc[1]), int(facing)))
    g = goals(m, D, K)
    return m, D, g, [-1 if p is None else D[p] for p in g]


def column_of(found, item, T, ids):
    """(the plan column [T] to `item`, its true length) of a searched state."""
    m, D, g, dist = found
    column = [-1] * T
    if g[item] is not None:
        moves = path(m, D, g[item], ids)
        assert len(moves) == dist[item]
        column[:min(len(moves), T)] = moves[:T]
    return column, dist[item]


def walk(map_row, loc, facing, K, item=None, T=None, ids=(0, 1, 2)):
    """One state's answer: (dist [K], plan column [T] or None, length or None)."""
    found = search(map_row, loc, facing, K)
    if item is None:
        return found[3], None, None
    return (found[3],) + column_of(found, item, T, ids)


def walk_rows(rows, idx, K, items=None, T=None, ids=(0, 1, 2)):
    """walk() of rows idx of a state dict (get_state() / Snapshot.state()) -> (dist int32 [n, K], plans int32 [T, n] or None, length int32 [n] or
    None); equal rows are walked once."""
    idx = [int(i) for i in idx]
    n = len(idx)
    dist = np.zeros((n, K), np.int32)
    plans = None if items is None else np.full((T, n), -1, np.int32)
    length = None if items is None else np.zeros(n, np.int32)
    seen = {}
    for j, i in enumerate(idx):
        if i not in seen:
            seen[i] = search(rows['map'][i], rows['loc'][i], rows['facing'][i], K)
        dist[j] = seen[i][3]
        if items is not None:
            plans[:, j], length[j] = column_of(seen[i], int(items[j]), T, ids)
    return dist, plans, length


def faces(rows, i, item):
    """Does the agent of row i face a cell of id `item`?"""
    cells = np.asarray(rows['map'][i]).reshape(-1)
    S = int(round(len(cells) ** 0.5))
    r, c, f = int(rows['loc'][i][0]), int(rows['loc'][i][1]), int(rows['facing'][i])
    fr, fc = r + DR[f], c + DC[f]
    return 0 <= fr < S and 0 <= fc < S and int(cells[fr * S + fc]) == item
