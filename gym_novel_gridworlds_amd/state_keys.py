"""State keys on the host: the 64-bit key contract of include/ngw.h (ngw_state_keys) in vectorised numpy, for users who key states they
hold in host memory (get_state() / Snapshot.state()).  The device computes the same keys without the copy: Snapshot.keys(),
VecNovelGridworld.state_keys().

    mix64(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31      (uint64, wrapping)
    term(tag, index, value) = mix64(tag << 56 | index << 32 | uint32(value))

and a key is the XOR of the terms of the selected fields (the table in include/ngw.h).  Keys depend on the state alone - not on the env
index, the slot or the rank - so they compare across snapshots, envs and processes."""
import numpy as np

KEY_MAP, KEY_POSE, KEY_INV, KEY_SELECTED, KEY_STEP_COUNT, KEY_EPISODE = 1, 2, 4, 8, 16, 32   # include/ngw.h NGW_KEY_*
KEY_STATE = 15            # map | pose | inventory | selected item: the Markov state with autoreset off
KEY_ALL = 63

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def check_fields(fields):
    """`fields` as an int: a non-empty selection of KEY_* bits, ValueError otherwise."""
    if isinstance(fields, bool) or not isinstance(fields, (int, np.integer)):
        raise ValueError("fields: a selection of KEY_* bits expected, got %r" % (fields,))
    f = int(fields)
    if f <= 0 or f & ~KEY_ALL:
        raise ValueError("fields: a non-empty selection of KEY_* bits (1 .. %d) expected, got %d" % (KEY_ALL, f))
    return f


def mix64(x):
    """The splitmix64 finaliser over a uint64 array (wrapping)."""
    x = np.asarray(x, np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= _M1
    x ^= x >> np.uint64(27)
    x *= _M2
    x ^= x >> np.uint64(31)
    return x


def terms(tag, index, value):
    """term(tag, index, value) elementwise: `index` and `value` broadcast, `value` is taken modulo 2^32."""
    v = np.asarray(value).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    head = np.uint64(tag << 56) | (np.asarray(index).astype(np.uint64) << np.uint64(32))
    return mix64(head | v)


def keys_of_rows(rows, fields=KEY_STATE):
    """The keys of the states in `rows` - a dict shaped like get_state() / Snapshot.state(): 'map' int8 [n, S*S] (or [n, S, S]), 'loc'
    [n, 2], 'facing', 'inv' [n, K], 'selected', 'step_count', 'episode' - as numpy uint64 [n], bit for bit what the device computes.
    Only the arrays of the selected fields are read."""
    f = check_fields(fields)
    n = None
    for name in ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode'):
        if name in rows and rows[name] is not None:
            n = len(rows[name])
            break
    if n is None:
        raise ValueError("rows: a dict of state arrays expected")
    key = np.zeros(n, np.uint64)
    with np.errstate(over='ignore'):
        if f & KEY_MAP:
            m = np.ascontiguousarray(rows['map'], np.int8).reshape(n, -1)
            groups = (m.shape[1] + 3) // 4
            cells = np.zeros((n, groups * 4), np.uint8)                 # cells past S*S count as 0
            cells[:, :m.shape[1]] = m.view(np.uint8)
            w = cells.view('<u4')                                       # [n, groups]: little-endian words of four cells
            t = terms(1, np.arange(groups, dtype=np.uint64)[None, :], w)
            key ^= np.bitwise_xor.reduce(np.where(w != 0, t, np.uint64(0)), axis=1)
        if f & KEY_POSE:
            loc = np.asarray(rows['loc']).astype(np.int64).reshape(n, 2)
            key ^= terms(2, 0, loc[:, 0] | loc[:, 1] << 8 | np.asarray(rows['facing']).astype(np.int64) << 16)
        if f & KEY_INV:
            inv = np.asarray(rows['inv']).astype(np.int64).reshape(n, -1)
            t = terms(3, np.arange(inv.shape[1], dtype=np.uint64)[None, :], inv)
            key ^= np.bitwise_xor.reduce(np.where(inv != 0, t, np.uint64(0)), axis=1)
        if f & KEY_SELECTED:
            key ^= terms(4, 0, rows['selected'])
        if f & KEY_STEP_COUNT:
            key ^= terms(5, 0, rows['step_count'])
        if f & KEY_EPISODE:
            key ^= terms(6, 0, rows['episode'])
    return key


def unique_of_keys(keys):
    """Groups of equal keys: (first, inverse) - inverse[j] is the group of position j, first[g] the smallest position in group g.  `keys`
    is a numpy array (np.unique) or a torch tensor (torch.unique and a scatter-amin: the result stays on its device, int64)."""
    if hasattr(keys, 'data_ptr'):
        import torch
        _, inverse = torch.unique(keys, return_inverse=True)
        n_groups = int(inverse.max().item()) + 1 if inverse.numel() else 0
        first = torch.full((n_groups,), keys.numel(), dtype=torch.int64, device=keys.device)
        first.scatter_reduce_(0, inverse, torch.arange(keys.numel(), dtype=torch.int64, device=keys.device), 'amin')
        return first, inverse
    _, first, inverse = np.unique(np.asarray(keys), return_index=True, return_inverse=True)
    return first.astype(np.int64), inverse.reshape(-1).astype(np.int64)
