"""The frontier contract of include/ngw.h (ngw_frontier_compact / ngw_frontier_alloc, NGW_IDX_NONE) restated with plain Python loops, written from the
contract text and not from gym_novel_gridworlds_amd/frontier.py (whose compact_reference / alloc_reference tests/test_frontier_oracle_cpu.py holds to
this).  The padded twins of the dense helpers (fresh_pairs, fresh_steps, transitions, tree_steps) are the same compaction of a [rows, div] flag array."""
import numpy as np

IDX_NONE = -(1 << 31)                # NGW_IDX_NONE INT32_MIN
F_FRONTIER_FULL = 32                 # NGW_F_FRONTIER_FULL


def compact(flags, div=1, map=None, capacity=None):
    """-> (first int32 [capacity], second int32 [capacity], [taken, total], full): the positions p of the non-zero bytes of `flags` (read flattened)
    in ascending order; entry k < taken = min(total, capacity) is (map[p // div] or p // div, p % div), IDX_NONE behind; full = total > capacity.
    capacity None: the number of hits."""
    raw = np.ascontiguousarray(flags).reshape(-1).view(np.uint8).tolist()
    hits = [p for p, b in enumerate(raw) if b != 0]
    total = len(hits)
    capacity = total if capacity is None else int(capacity)
    taken = min(total, capacity)
    first, second = [IDX_NONE] * capacity, [IDX_NONE] * capacity
    for k in range(taken):
        p = hits[k]
        first[k] = int(map[p // div]) if map is not None else p // div
        second[k] = p % div
    return np.array(first, np.int32).reshape(capacity), np.array(second, np.int32).reshape(capacity), [taken, total], total > capacity


def alloc(count, cursor, limit, capacity):
    """-> (slots int32 [capacity], the cursor afterwards, full): m = max(min(count, limit - cursor), 0); slot k is cursor + k for k < m, IDX_NONE
    behind; the cursor moves on by m; full = m < count."""
    m = max(min(int(count), int(limit) - int(cursor)), 0)
    slots = [IDX_NONE] * int(capacity)
    for k in range(min(m, int(capacity))):
        slots[k] = int(cursor) + k
    return np.array(slots, np.int32).reshape(int(capacity)), int(cursor) + m, m < int(count)
