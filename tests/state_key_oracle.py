"""The state-key contract of include/ngw.h (ngw_state_keys) restated with plain Python integers: one row at a time, one cell at a time,
masked to 64 bits by hand.  Deliberately unlike both the kernel (csrc/ngw_keys.inc: 16 lanes per row, DPP reduction) and the numpy twin
(state_keys.keys_of_rows: whole arrays, wrapping uint64)."""
import numpy as np

M64 = (1 << 64) - 1
MAP, POSE, INV, SELECTED, STEP_COUNT, EPISODE = 1, 2, 4, 8, 16, 32
STATE, ALL = 15, 63
SINGLE = (MAP, POSE, INV, SELECTED, STEP_COUNT, EPISODE)
FIELD_OF = {'map': MAP, 'loc': POSE, 'facing': POSE, 'inv': INV, 'selected': SELECTED, 'step_count': STEP_COUNT, 'episode': EPISODE}


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def term(tag, index, value):
    return mix64((tag << 56) | (index << 32) | (int(value) & 0xFFFFFFFF))


def map_group_word(cells, g):
    """The little-endian word of cells 4g .. 4g+3 of one row's cells (a sequence of ints); cells past the end count as 0."""
    w = 0
    for b in range(4):
        i = 4 * g + b
        if i < len(cells):
            w |= (int(cells[i]) & 0xFF) << (8 * b)
    return w


def key_of_row(rows, i, fields):
    """The key of row i of a dict shaped like get_state() / Snapshot.state()."""
    assert 0 < fields <= ALL
    key = 0
    if fields & MAP:
        cells = [int(c) for c in np.asarray(rows['map'][i]).reshape(-1)]
        for g in range((len(cells) + 3) // 4):
            w = map_group_word(cells, g)
            if w:
                key ^= term(1, g, w)
    if fields & POSE:
        r, c, f = int(rows['loc'][i][0]), int(rows['loc'][i][1]), int(rows['facing'][i])
        key ^= term(2, 0, r | c << 8 | f << 16)
    if fields & INV:
        for k, q in enumerate(np.asarray(rows['inv'][i]).reshape(-1)):
            if int(q):
                key ^= term(3, k, int(q))
    if fields & SELECTED:
        key ^= term(4, 0, int(rows['selected'][i]))
    if fields & STEP_COUNT:
        key ^= term(5, 0, int(rows['step_count'][i]))
    if fields & EPISODE:
        key ^= term(6, 0, int(rows['episode'][i]))
    return key


class Table:
    """The keys of the rows of one dict of state arrays, each row hashed at most once per single field (a key under several fields is the
    XOR of its single-field keys: the definition), so that a test can ask for many selections and index lists of the same rows."""

    def __init__(self, rows):
        self.rows, self.memo = rows, {}

    def key(self, i, fields):
        assert 0 < fields <= ALL
        key = 0
        for bit in SINGLE:
            if fields & bit:
                if (i, bit) not in self.memo:
                    self.memo[(i, bit)] = key_of_row(self.rows, i, bit)
                key ^= self.memo[(i, bit)]
        return key


def keys_of(rows, idx, fields):
    """uint64 [len(idx)]: the key of row idx[j] of `rows` (a dict of state arrays, or a Table over one)."""
    table = rows if isinstance(rows, Table) else Table(rows)
    return np.array([table.key(int(i), fields) for i in idx], np.uint64).reshape(len(idx))


def as_u64(got):
    """The keys a call returned (numpy uint64, or a torch int64 tensor over the same bits) as numpy uint64."""
    if hasattr(got, 'data_ptr'):
        import torch
        assert got.dtype == torch.int64, got.dtype
        return got.cpu().numpy().view(np.uint64)
    got = np.asarray(got)
    assert got.dtype == np.uint64, got.dtype
    return got


def assert_keys(got, rows, idx, fields, where):
    got = as_u64(got)
    exp = keys_of(rows, idx, fields)
    assert got.shape == exp.shape, (where, got.shape, exp.shape)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, "%s, fields %d: %d of %d keys differ, first at position %d (row %d): got %#018x, expected %#018x" % (
        where, fields, bad.size, exp.size, bad[0], int(idx[bad[0]]), int(got[bad[0]]), int(exp[bad[0]]))
