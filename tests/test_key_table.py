"""The device-side key table and Snapshot.copy on the MI355X (csrc/ngw_table.inc, include/ngw.h ngw_key_table_* / ngw_snapshot_copy;
key_table.py, Snapshot.copy / insert_keys).  `fresh` is held exactly to the model of tests/key_table_oracle.py - a Python dict from key to
first-seen order -, `where` to its properties only (which bucket a key gets is not part of the contract); copies to a host copy of the
source rows; the breadth-first search to the same search run with the CPU oracle and a Python set."""
import numpy as np
import pytest

import expand_oracle as XO
import key_table_oracle as KT
import ngw_testlib as T
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.key_table import KeyInsert
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_TABLE_FULL, make_spec
from gym_novel_gridworlds_amd.state_keys import keys_of_rows

pytestmark = pytest.mark.gpu
S_SMALL = 9                     # the smallest map size tests/test_expand.py uses; S * S = 81 is odd


def dev_i32(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def distinct_keys(n, salt=0):
    """n distinct non-zero uint64 keys (an odd multiplier permutes the 64-bit integers)."""
    with np.errstate(over='ignore'):
        k = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(salt << 20)) * np.uint64(0x9E3779B97F4A7C15)
    assert len(set(k.tolist())) == n and (k != 0).all()
    return k


@pytest.fixture(scope='module')
def venv():
    """One small env for every table test: a table needs its env's stream and flags word, never its states."""
    spec = make_spec(T.POGO, S_SMALL)
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=XO.good_seed(spec, 4))
    v.reset()
    yield v
    v.close()


def offer(table, model, book, keys, what, device=False):
    """One insert held to the model and the book; -> the KeyInsert as numpy arrays."""
    exp_fresh, stored = model.insert(keys)
    got = table.insert(keys, device=device)
    assert isinstance(got, KeyInsert)
    where, fresh = (got.where.cpu().numpy(), got.fresh.cpu().numpy()) if device else got
    assert fresh.dtype == np.bool_ and fresh.shape == exp_fresh.shape, (what, fresh.dtype, fresh.shape)
    bad = np.nonzero(fresh != exp_fresh)[0]
    assert bad.size == 0, "%s: fresh differs at %d positions, first %d: got %r" % (what, bad.size, bad[0], bool(fresh[bad[0]]))
    book.check(keys, where, stored, what)
    return KeyInsert(where, fresh)


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 130])
def test_distinct_keys_around_the_wave_boundary(venv, count):
    """A partial wave, the wave boundary, and - at 130 of 256 lanes - the later waves of a work-group; then the same keys again."""
    table = venv.key_table(256)
    assert table.capacity == 256 and table.buckets == 512 and len(table) == 0
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = distinct_keys(count, salt=count)
    first = offer(table, model, book, keys, 'first call')
    assert first.fresh.all() and len(table) == count
    assert (table.lookup(keys) == first.where).all()
    again = offer(table, model, book, keys, 'second call')
    assert not again.fresh.any() and (again.where == first.where).all() and len(table) == count
    assert venv.error_flags() == 0
    table.close()


def test_two_work_groups(venv):
    """600 distinct keys: three work-groups of 256 lanes, the last one partial."""
    table = venv.key_table(1024)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = distinct_keys(600, salt=3)
    got = offer(table, model, book, keys, '600 keys')
    assert got.fresh.all() and len(set(got.where.tolist())) == 600 and len(table) == 600
    assert venv.error_flags() == 0
    table.close()


def test_copies_of_one_key(venv):
    """200 lanes fight for one bucket: only position 0 is fresh, every `where` is that bucket, one key is stored."""
    table = venv.key_table(64)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    got = offer(table, model, book, np.full(200, 0xDEADBEEFCAFEF00D, np.uint64), '200 copies')
    assert got.fresh.tolist() == [True] + [False] * 199 and (got.where == got.where[0]).all() and len(table) == 1
    assert venv.error_flags() == 0
    table.close()


def test_one_key_in_two_waves(venv):
    """The same key at positions 3 and 200 - different waves - among distinct ones: fresh at 3, whichever wave ran first."""
    table = venv.key_table(512)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = distinct_keys(260, salt=5)
    keys[200] = keys[3]
    got = offer(table, model, book, keys, 'positions 3 and 200')
    assert got.fresh[3] and not got.fresh[200] and got.where[3] == got.where[200] and int(got.fresh.sum()) == 259 and len(table) == 259
    assert venv.error_flags() == 0
    table.close()


@pytest.mark.parametrize('device', [False, True])
def test_keys_that_catch_a_32_bit_compare_or_an_all_ones_mark(venv, device):
    """1, 2^64 - 1, 2^32, 2^32 | 1, two keys equal in the low 32 bits and two equal in the high 32 bits are eight different keys."""
    import torch
    special = np.array([1, (1 << 64) - 1, 1 << 32, (1 << 32) | 1, 0xAAAA000000000007, 0xBBBB000000000007, 0x1234567800000001, 0x1234567800000002],
                       np.uint64)
    table = venv.key_table(16)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = torch.from_numpy(special.view(np.int64)).cuda() if device else special
    got = offer(table, model, book, keys, 'special keys', device=device)
    assert got.fresh.all() and len(set(got.where.tolist())) == 8 and len(table) == 8
    absent = np.array([2, 2 << 32, (1 << 64) - 2, 0x0000000000000007, 0x1234567800000000, 0], np.uint64)
    found = table.lookup(np.concatenate([special, absent]))
    assert (found[:8] == got.where).all() and (found[8:] == -1).all()
    assert not offer(table, model, book, keys, 'special keys again', device=device).fresh.any() and len(table) == 8
    assert venv.error_flags() == 0
    table.close()


def test_key_zero_is_never_stored(venv):
    table = venv.key_table(16)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    got = offer(table, model, book, np.array([5, 0, 6, 0, 5], np.uint64), 'zeros mixed in')
    assert got.where[1] == got.where[3] == -1 and got.fresh.tolist() == [True, False, True, False, False] and len(table) == 2
    got = offer(table, model, book, np.zeros(70, np.uint64), 'only zeros')
    assert (got.where == -1).all() and not got.fresh.any() and len(table) == 2
    assert table.lookup([0, 5]).tolist() == [-1, int(table.lookup([5])[0])] and table.lookup([5])[0] >= 0
    assert venv.error_flags() == 0                                   # key 0 raises no flag
    table.close()


def test_three_calls_against_the_model(venv):
    """5 000 draws from 700 distinct values into capacity 1024, three times: fresh equals the model on every call, keys of earlier calls
    keep their buckets, lookup agrees with insert and with the model, a key never inserted looks up as -1."""
    rs = np.random.RandomState(11)
    values = distinct_keys(700, salt=7)
    never = distinct_keys(50, salt=9)
    assert not set(never.tolist()) & set(values.tolist())
    table = venv.key_table(1024)
    assert table.buckets == 2048
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    draws = values[rs.randint(0, 700, 5000)]
    for call, keys in enumerate((draws[:1500], draws[1500:3200], draws[3200:])):      # (the first call leaves values for the later ones to bring)
        before = len(model)
        offer(table, model, book, keys, 'call %d' % call)
        assert len(model) > before
        assert len(table) == len(model)
        found = table.lookup(np.concatenate([values, never]))
        held = model.contains(values)
        assert (found[:700][~held] == -1).all() and (found[700:] == -1).all()
        book.check(values[held], found[:700][held], np.ones(int(held.sum()), bool), 'lookup after call %d' % call)
    assert len(model) > 600
    assert venv.error_flags() == 0
    table.close()


def test_forced_probing_wrap_around_and_a_full_table(venv):
    """capacity 4 = 8 buckets, 12 distinct keys: exactly 8 are stored, in 8 different buckets, and are fresh; 4 are refused (-1, not fresh,
    F_TABLE_FULL).  Which 4 is not asserted.  The 8 stored keys then find their buckets again, without a flag."""
    table = venv.key_table(4)
    assert table.buckets == 8
    keys = distinct_keys(12, salt=13)
    assert venv.error_flags() == 0
    where, fresh = table.insert(keys)
    stored = where >= 0
    assert int(stored.sum()) == 8 and sorted(where[stored].tolist()) == list(range(8)) and (where[~stored] == -1).all()
    assert (fresh == stored).all() and len(table) == 8
    assert venv.error_flags() == F_TABLE_FULL and venv.error_flags() == 0
    again = table.insert(keys[stored])
    assert not again.fresh.any() and (again.where == where[stored]).all() and len(table) == 8
    assert venv.error_flags() == 0
    found = table.lookup(keys)                                        # a lookup in a full table ends after one round, too
    assert (found == where).all()
    assert venv.error_flags() == 0                                   # (a lookup raises nothing)
    table.close()


def test_clear(venv):
    table = venv.key_table(128)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = distinct_keys(100, salt=17)
    offer(table, model, book, keys, 'before clear')
    assert len(table) == 100
    table.clear()
    assert len(table) == 0 and (table.lookup(keys) == -1).all()
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    assert offer(table, model, book, keys, 'after clear').fresh.all() and len(table) == 100
    assert venv.error_flags() == 0
    table.close()
    with pytest.raises(ValueError, match='closed'):
        table.insert(keys)


def test_the_device_path_and_insert_keys(venv):
    """Keys straight from Snapshot.keys(device=True); the results are tensors; insert_keys equals keys + insert; the envs' own keys."""
    import torch
    n = venv.num_envs
    pool = venv.snapshot(64)
    pool.save(slots=np.arange(n))
    pool.expand(np.arange(60) % n, np.arange(60) % venv.n_actions, 4 + np.arange(60), from_envs=True)      # some states twice
    slots = np.arange(64)
    table, twin = venv.key_table(64), venv.key_table(64)
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    keys = pool.keys(slots, device=True)
    got = table.insert(keys, device=True)
    assert isinstance(got.where, torch.Tensor) and got.where.dtype == torch.int32 and got.where.is_cuda and tuple(got.where.shape) == (64,)
    assert isinstance(got.fresh, torch.Tensor) and got.fresh.dtype == torch.bool and got.fresh.is_cuda and tuple(got.fresh.shape) == (64,)
    host_keys = KT.as_u64(keys)
    assert (host_keys == keys_of_rows(pool.state())).all()
    exp_fresh, stored = model.insert(host_keys)
    assert (got.fresh.cpu().numpy() == exp_fresh).all() and 1 < int(exp_fresh.sum()) < 64
    book.check(host_keys, got.where, stored, 'device path')
    assert (table.lookup(keys, device=True).cpu().numpy() == got.where.cpu().numpy()).all()
    k2, ins2 = pool.insert_keys(twin, slots, device=True)            # the same batch into an empty twin: the same keys, the same fresh
    assert isinstance(k2, torch.Tensor) and (KT.as_u64(k2) == host_keys).all() and (ins2.fresh.cpu().numpy() == exp_fresh).all()
    KT.WhereBook(twin.buckets).check(host_keys, ins2.where, stored, 'insert_keys')
    k3, ins3 = pool.insert_keys(twin)                                 # host results, every slot: nothing is new
    assert isinstance(k3, np.ndarray) and k3.dtype == np.uint64 and (k3 == host_keys).all() and not ins3.fresh.any()
    assert (ins3.where == ins2.where.cpu().numpy()).all() and len(twin) == len(table) == len(model)
    ke, inse = venv.insert_state_keys(table)                          # the envs' states are slots 0 .. n-1: all seen
    assert (ke == venv.state_keys()).all() and (ke == host_keys[:n]).all() and not inse.fresh.any()
    assert (inse.where == got.where.cpu().numpy()[:n]).all()
    with pytest.raises(ValueError, match='another env'):
        other = VecNovelGridworld(spec=venv.spec, num_envs=2, seed=1)
        try:
            pool.insert_keys(other.key_table(4))
        finally:
            other.close()
    assert venv.error_flags() == 0
    for x in (table, twin, pool):
        x.close()


def test_tables_close_with_the_env():
    spec = make_spec(T.POGO, S_SMALL)
    v = VecNovelGridworld(spec=spec, num_envs=2, seed=XO.good_seed(spec, 2))
    v.reset()
    a, b = v.key_table(8), v.key_table(8)
    a.insert([1, 2, 3])
    a.close()
    assert a.closed and not b.closed
    v.rebuild(spec)                                                  # an in-place rebuild closes what is open
    assert b.closed
    with pytest.raises(ValueError, match='closed'):
        b.insert([1])
    v.reset()
    c = v.key_table(8)
    assert c.insert([4, 4]).fresh.tolist() == [True, False]
    v.close()
    with pytest.raises(ValueError, match='closed'):
        len(c)


def _played_env(S, n):
    spec = make_spec(T.POGO, S)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=XO.good_seed(spec, n), autoreset=True, horizon=5)
    v.reset()
    rs = np.random.RandomState(S)
    for t in range(13):                                              # (two horizons and three steps: episode counters and step counts are not 0)
        v.step(rs.randint(0, len(spec.actions_id), n).astype(np.int32))
    return v


def _expect_copy(before_dst, src_rows, src_slots, dst_slots):
    exp = {k: x.copy() for k, x in before_dst.items()}
    for k in XO.STATE_KEYS:
        exp[k][np.asarray(dst_slots)] = src_rows[k][np.asarray(src_slots)]
    return exp


@pytest.mark.parametrize('S', [S_SMALL, 10])
def test_snapshot_copy(S):
    """Within one pool and across two, with lists and with device tensors: the destinations hold the sources' rows field by field, episode
    counter included; every other slot is unchanged; a bad device index skips its pair and raises F_BAD_INDEX."""
    n = 6
    v = _played_env(S, n)
    pool, other = v.snapshot(16), v.snapshot(8)
    pool.save(slots=np.arange(n))
    assert (pool.state()['episode'][:n] >= 2).all() and (pool.state()['step_count'][:n] > 0).all()
    # inside one pool, host lists, a source twice
    before = pool.state()
    pool.copy([0, 1, 1, 5], [8, 9, 10, 15])
    XO.assert_rows(pool.state(), _expect_copy(before, before, [0, 1, 1, 5], [8, 9, 10, 15]), 'S=%d one pool, lists' % S)
    # across two pools
    src, before = pool.state(), other.state()
    other.copy([3, 0, 9], [7, 2, 4], source=pool)
    XO.assert_rows(other.state(), _expect_copy(before, src, [3, 0, 9], [7, 2, 4]), 'S=%d two pools, lists' % S)
    XO.assert_rows(pool.state(), src, 'S=%d two pools: the source' % S)
    # device tensors, inside one pool and across
    before = pool.state()
    pool.copy(dev_i32([2, 4]), dev_i32([11, 12]))
    XO.assert_rows(pool.state(), _expect_copy(before, before, [2, 4], [11, 12]), 'S=%d one pool, tensors' % S)
    src, before = other.state(), pool.state()
    pool.copy(dev_i32([7, 2]), dev_i32([13, 14]), source=other)
    XO.assert_rows(pool.state(), _expect_copy(before, src, [7, 2], [13, 14]), 'S=%d two pools, tensors' % S)
    # one list only; no list at all
    src, before = pool.state(), other.state()
    other.copy(None, [6, 5], source=pool)                            # slots 0, 1 of the pool
    XO.assert_rows(other.state(), _expect_copy(before, src, [0, 1], [6, 5]), 'S=%d no source list' % S)
    whole = v.snapshot(16)
    whole.copy(None, None, source=pool)
    XO.assert_rows(whole.state(), pool.state(), 'S=%d without lists' % S)
    assert v.error_flags() == 0
    # bad device indices: a source beyond its pool, a destination beyond its own, a negative one
    src, before = other.state(), pool.state()
    pool.copy(dev_i32([0, 8, 1, 2, -1]), dev_i32([3, 4, 16, 6, 5]), source=other)
    XO.assert_rows(pool.state(), _expect_copy(before, src, [0, 2], [3, 6]), 'S=%d bad indices' % S)
    assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
    with pytest.raises(ValueError, match='also a source'):
        pool.copy([0, 1], [1, 2])
    with pytest.raises(ValueError, match='twice'):
        pool.copy([0, 1], [2, 2])
    XO.assert_rows(pool.state(), _expect_copy(before, src, [0, 2], [3, 6]), 'S=%d refused calls' % S)
    v.close()


def test_breadth_first_search_closes_on_the_device():
    """Depth 3 from one env's reset state: expand_all into a scratch pool, insert_keys, copy of the fresh children into an archive pool.  The
    CPU side runs the same search with the oracle's expand, keys_of_rows and a Python set: at every depth the number of fresh states and the
    set of their keys match; at the end len(table) is the size of the set and the archive's filled slots hold exactly those keys."""
    spec = make_spec(T.POGO, S_SMALL)
    v = VecNovelGridworld(spec=spec, num_envs=2, seed=XO.good_seed(spec, 2))
    v.reset()
    A = v.n_actions
    total = 1 + A + A * A + A ** 3
    archive, scratch, table = v.snapshot(total), v.snapshot(A ** 3), v.key_table(total)
    # the device side's root
    archive.save(envs=[0], slots=[0])
    keys, ins = archive.insert_keys(table, [0])
    assert ins.fresh.tolist() == [True]
    frontier, filled = np.array([0]), 1
    # the CPU side's root
    root = v.get_state()
    rows = {k: np.asarray(root[k])[:1].reshape(1, -1) if k in ('map', 'loc', 'inv') else np.asarray(root[k])[:1] for k in XO.STATE_KEYS}
    seen = {int(keys_of_rows(rows)[0])}
    assert int(keys[0]) in seen
    for depth in range(1, 4):
        P = len(frontier)
        scratch.expand_all(frontier, 0, source=archive)
        keys, ins = scratch.insert_keys(table, np.arange(P * A))
        new = np.nonzero(ins.fresh)[0]
        archive.copy(new, filled + np.arange(len(new)), source=scratch)
        frontier, filled = filled + np.arange(len(new)), filled + len(new)
        # the same level on the CPU: every frontier row with every action, parent-major as expand_all orders its children
        children, _ = XO.oracle_expand(spec, rows, np.repeat(np.arange(len(rows['loc'])), A), np.tile(np.arange(A), len(rows['loc'])))
        ckeys = keys_of_rows(children)
        fresh_cpu = []
        for j, k in enumerate(ckeys.tolist()):
            if k not in seen:
                seen.add(k)
                fresh_cpu.append(j)
        assert len(rows['loc']) == P and (keys == ckeys).all(), "depth %d: the children's keys differ" % depth
        assert len(new) == len(fresh_cpu) and set(keys[new].tolist()) == set(ckeys[fresh_cpu].tolist()), "depth %d" % depth
        assert new.tolist() == fresh_cpu                             # (and, both being first occurrences, the same positions)
        rows = {k: np.asarray(children[k])[fresh_cpu].reshape(len(fresh_cpu), -1) if k in ('map', 'loc', 'inv') else np.asarray(children[k])[fresh_cpu]
                for k in XO.STATE_KEYS}
        assert len(fresh_cpu) > 0
    assert len(table) == len(seen) == filled
    held = archive.keys(np.arange(filled))
    assert len(set(held.tolist())) == filled and set(held.tolist()) == seen
    assert (table.lookup(held) >= 0).all()
    assert v.error_flags() == 0
    v.close()
