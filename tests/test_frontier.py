"""Device-side frontiers on the MI355X (csrc/ngw_frontier.inc, include/ngw.h ngw_frontier_compact / ngw_frontier_alloc / NGW_IDX_NONE,
frontier.Frontier): compaction and allocation against their numpy statements, the skipped pair in every call that takes a device index list -
against the same call with a bad index, with a valid index and on the live entries alone -, and a breadth-first search written with and without
a host round trip per iteration."""
import numpy as np
import pytest

import expand_oracle as XO
from gym_novel_gridworlds_amd import VecNovelGridworld, frontier as F
from gym_novel_gridworlds_amd.lidar import LidarConfig
from gym_novel_gridworlds_amd.snapshot import fresh_pairs
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, F_FRONTIER_FULL, IDX_NONE, make_spec

pytestmark = pytest.mark.gpu
TILE = 4096                          # csrc/ngw_device.h NGW_FRONTIER_TILE
N_ENVS = 64


def dev(x, dtype=np.int32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()
    torch.cuda.synchronize()
    return t


def host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


@pytest.fixture(scope='module')
def world():
    """One 10 x 10 Pogostick-v1 handle of 64 envs after 30 random steps, lidar configured; a pool of 512 slots whose first 128 hold the envs'
    states and a generation of children of them."""
    spec = make_spec('NovelGridworld-Pogostick-v1', 10)
    v = VecNovelGridworld(spec=spec, num_envs=N_ENVS, seed=XO.good_seed(spec, N_ENVS), autoreset=True, horizon=40)
    v.reset()
    rs = np.random.RandomState(5)
    A = len(spec.actions_id)
    for _ in range(30):
        v.step(rs.randint(0, A, N_ENVS).astype(np.int32))
    v.lidar_configure(LidarConfig(spec, 8), dtype=np.int32)
    pool = v.snapshot(512)
    pool.save(slots=np.arange(N_ENVS))
    pool.expand(rs.randint(0, N_ENVS, N_ENVS), rs.randint(0, A, N_ENVS), N_ENVS + np.arange(N_ENVS))
    v.sync()
    assert v.error_flags() == 0
    yield v, pool, spec
    v.close()


# ---------------------------------------------------------------------------------------------------------------- compaction
def flag_cases(n, rs):
    yield 'none', np.zeros(n, np.uint8)
    yield 'all', np.ones(n, np.uint8)
    f = (rs.randint(0, 17, n) == 0).astype(np.uint8)
    yield 'sparse', f
    g = f.copy()
    if n:
        g[rs.randint(0, n, 6)] = np.array([2, 0x80, 0xFF, 2, 0x80, 0xFF], np.uint8)      # any non-zero byte counts
    yield 'stray', g


@pytest.mark.parametrize('n', [0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 64 * 17])
def test_compaction_against_the_reference(world, n):
    import torch
    v, pool, _ = world
    rs = np.random.RandomState(100 + n)
    for name, flags in flag_cases(n, rs):
        total = int(np.count_nonzero(flags))
        fd = dev(flags, np.uint8)
        for div in (1, 17):
            amap = (rs.permutation(-(-n // div) + 3) + 7).astype(np.int32)
            for m in (None, amap):
                md = None if m is None else dev(m)
                for cap in sorted({max(total - 1, 0), total, total + 70}):
                    where = 'n %d %s div %d map %s capacity %d' % (n, name, div, m is not None, cap)
                    fr = pool.frontier(cap)
                    first, second = fr.compact(fd, div, md)
                    e_first, e_second, e_count, e_full = F.compact_reference(flags, div, m, cap)
                    assert first.dtype == second.dtype == torch.int32 and first.shape == second.shape == (cap,), where
                    assert (host(first) == e_first).all() and (host(second) == e_second).all(), where
                    assert (host(first)[min(total, cap):] == IDX_NONE).all(), where
                    assert (host(fr.count_dev) == e_count).all() and fr.count() == min(total, cap) and fr.total() == total, where
                    assert v.error_flags() == (F_FRONTIER_FULL if e_full else 0), where
                    fr.close()
    # bool flags of two dimensions read flattened; the same input twice: the same bytes
    flags = (rs.randint(0, 5, n) == 0)
    fr, fr2 = pool.frontier(n + 3), pool.frontier(n + 3)
    a, b = fr.compact(dev(flags, np.bool_).reshape(1, -1), 17)
    a2, b2 = fr2.compact(dev(flags, np.bool_).reshape(1, -1), 17)
    e = F.compact_reference(flags, 17, None, n + 3)
    assert (host(a) == e[0]).all() and (host(b) == e[1]).all()
    assert host(a).tobytes() == host(a2).tobytes() and host(b).tobytes() == host(b2).tobytes() and host(fr.count_dev).tobytes() == host(fr2.count_dev).tobytes()
    assert v.error_flags() == 0


def test_compaction_without_second_and_misaligned_flags(world):
    """second_dev == NULL through the C-ABI; a flag array that starts one byte off a 16-byte boundary takes the byte loads."""
    import ctypes as C
    import torch
    from gym_novel_gridworlds_amd import _cabi
    v, pool, _ = world
    rs = np.random.RandomState(3)
    n = TILE + 77
    flags = (rs.randint(0, 9, n + 1) == 0).astype(np.uint8)
    fd = dev(flags, np.uint8)
    for off in (0, 1):
        f = flags[off:off + n]
        total = int(np.count_nonzero(f))
        first = torch.full((total + 5,), 123, dtype=torch.int32, device='cuda')
        count = torch.zeros(2, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        rc = _cabi.lib().ngw_frontier_compact(v._h, C.c_void_p(fd.data_ptr() + off), n, 17, None, total + 5, C.c_void_p(first.data_ptr()), None,
                                              C.c_void_p(count.data_ptr()))
        assert rc == 0
        v.sync()
        e = F.compact_reference(f, 17, None, total + 5)
        assert (host(first) == e[0]).all() and (host(count) == e[2]).all()
        fr = pool.frontier(total + 5)
        a, b = fr.compact(fd[off:off + n], 17)
        assert (host(a) == e[0]).all() and (host(b) == e[1]).all()
    assert v.error_flags() == 0


def test_the_largest_frontier(world):
    """n = 65 536 x 17 at density 1 / 17."""
    v, pool, _ = world
    rs = np.random.RandomState(11)
    flags = (rs.randint(0, 17, (65536, 17)) == 0).astype(np.uint8)
    amap = rs.permutation(65536).astype(np.int32)
    fr = pool.frontier(70000)
    a, b = fr.compact(dev(flags, np.uint8), 17, dev(amap))
    e = F.compact_reference(flags, 17, amap, 70000)
    assert (host(a) == e[0]).all() and (host(b) == e[1]).all() and (host(fr.count_dev) == e[2]).all()
    assert v.error_flags() == 0


def test_python_argument_checks(world):
    import torch
    v, pool, _ = world
    fr = pool.frontier(8)
    ok = torch.ones(8, dtype=torch.uint8, device='cuda')
    for bad in (np.ones(8, np.uint8), torch.ones(8, dtype=torch.int32, device='cuda'), torch.ones(8, dtype=torch.uint8), ok[::2]):
        with pytest.raises(ValueError, match='flags'):
            fr.compact(bad)
    with pytest.raises(ValueError, match='div'):
        fr.compact(ok, 0)
    with pytest.raises(ValueError, match='map'):
        fr.compact(ok, 1, torch.zeros(8, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='map'):
        fr.compact(ok, 1, torch.zeros(7, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='capacity'):
        pool.frontier(-1)
    with pytest.raises(ValueError, match='limit'):
        fr.alloc(-1)
    fr.close()
    with pytest.raises(ValueError, match='closed'):
        fr.compact(ok)
    assert v.error_flags() == 0


# ---------------------------------------------------------------------------------------------------------------- allocation
@pytest.mark.parametrize('cursor, limit', [(0, 512), (37, 512), (0, 9), (3, 12), (3, 11), (3, 4), (12, 12), (20, 12)])
def test_allocation(world, cursor, limit):
    """9 hits in a list of 16: cursor 0 and not 0, the limit reached exactly (3 + 9 = 12), passed by one, nearly and already exhausted."""
    v, pool, _ = world
    flags = np.zeros(40, np.uint8)
    flags[[1, 2, 3, 5, 8, 13, 21, 34, 39]] = 1
    fr = pool.frontier(16)
    fr.reset_cursor(cursor)
    fr.compact(dev(flags, np.uint8))
    slots = fr.alloc(limit)
    e_slots, e_cursor, e_full = F.alloc_reference(9, cursor, limit, 16)
    assert (host(slots) == e_slots).all() and int(host(fr.cursor)[0]) == e_cursor
    assert v.error_flags() == (F_FRONTIER_FULL if e_full else 0)
    live = host(slots)[host(slots) != IDX_NONE]
    assert (live < limit).all()
    # the default limit is the pool's capacity; a second allocation goes on from the cursor
    fr.reset_cursor(500)
    s2 = host(fr.alloc()).copy()
    s3 = host(fr.alloc()).copy()
    assert (s2[:9] == 500 + np.arange(9)).all() and (s2[9:] == IDX_NONE).all()
    assert (s3[:3] == 509 + np.arange(3)).all() and (s3[3:] == IDX_NONE).all() and int(host(fr.cursor)[0]) == 512
    assert v.error_flags() == F_FRONTIER_FULL


def test_allocation_of_many_work_groups(world):
    """A list of several work-groups: every one of them reads the cursor before the last one writes it."""
    v, pool, _ = world
    n = 20000
    fr = pool.frontier(n + 100)
    fr.compact(dev(np.ones(n, np.uint8), np.uint8))
    for start in (7, 7 + n):
        fr.reset_cursor(7) if start == 7 else None
        e_slots, e_cursor, _ = F.alloc_reference(n, start, 1 << 30, n + 100)
        assert (host(fr.alloc(1 << 30)) == e_slots).all() and int(host(fr.cursor)[0]) == e_cursor
    assert v.error_flags() == 0


# ---------------------------------------------------------------------------------------------------------------- skipped pairs
COUNT = 130
LAYOUTS = {
    # about a third, across the boundary of the first two waves, and the whole last work-group (pairs 128, 129)
    'third': np.r_[5, 17, 40:70, 100:110, 128, 129],
    # the whole second work-group and a few beside it
    'block': np.r_[3, 64:128, 129],
}


def leaves(x):
    """The arrays of a result, in a fixed order."""
    if x is None:
        return []
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in leaves(x[k])]
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in leaves(y)]
    return [host(x)]


def pair_axis(a, count):
    return [i for i, s in enumerate(a.shape) if s == count][0]


def calls(world):
    """name -> (run(src, dst) -> (result, the destination rows afterwards or None), whether it has a destination, whether the dense call's
    rows are comparable (no draw by pair number)).  src indexes the pool's first 128 slots (save: the envs), dst slots 200 .. of the pool
    (restore: the envs)."""
    import torch
    v, pool, spec = world
    A, K = len(spec.actions_id), len(spec.items_id)
    rs = np.random.RandomState(9)
    acts = rs.randint(0, A, 4 * COUNT).astype(np.int32)
    items = rs.randint(0, K, 4 * COUNT).astype(np.int32)
    weights = rs.rand(A, 4 * COUNT).astype(np.float32)

    def col(x, src):                                  # per-pair inputs follow the pair's position in the list
        return x[..., :len(src)]

    def pool_rows():
        v.sync()
        return pool.state()

    def env_rows():
        v.sync()
        return v.get_state()

    def plans(src):
        return dev(np.ascontiguousarray(col(acts.reshape(4, -1)[:, :COUNT], src)))

    def moved(fn, rows):
        def run(s, d):
            fn(s, d)
            return None, rows()
        return run

    return {
        'save': (moved(lambda s, d: pool.save(envs=dev(s), slots=dev(d)), pool_rows), True, False),
        'restore': (moved(lambda s, d: pool.restore(slots=dev(s), envs=dev(d)), env_rows), True, False),
        'copy': (moved(lambda s, d: pool.copy(dev(s), dev(d)), pool_rows), True, False),
        'expand': (lambda s, d: (pool.expand(dev(s), dev(col(acts, s)), dev(d), device=True), pool_rows()), True, True),
        'rollout': (lambda s, d: (pool.rollout(dev(s), plans(s), dev(d), device=True), pool_rows()), True, True),
        'rollout_path_keys': (lambda s, d: (pool.rollout(dev(s), plans(s), dev(d), device=True, path_keys=True), pool_rows()), True, True),
        'rollout_rewards': (lambda s, d: (pool.rollout(dev(s), plans(s), None, device=True, rewards=True, observe='lidar'), None), False, True),
        'playout': (lambda s, d: (pool.playout(dev(s), 4, 77, dev(d), record=True, device=True, rewards=True, masks=True, path_keys=True,
                                               observe='agent_view'), pool_rows()), True, False),
        'keys': (lambda s, d: (pool.keys(dev(s), device=True), None), False, True),
        'successor_keys': (lambda s, d: (pool.successor_keys(dev(s), device=True), None), False, True),
        'sample_actions': (lambda s, d: (pool.sample_actions(dev(s), dev(col(weights, s), np.float32), 5, device=True), None), False, False),
        'lidar_observation': (lambda s, d: (pool.lidar_observation(dev(s), device=True), None), False, True),
        'agent_view': (lambda s, d: (pool.agent_view(dev(s), device=True), None), False, True),
        'action_masks': (lambda s, d: (pool.action_masks(dev(s), device=True), None), False, True),
        'walk_distances': (lambda s, d: (pool.walk_distances(dev(s), device=True), None), False, True),
        'walk_plans': (lambda s, d: (pool.walk_plans(dev(s), dev(col(items, s)), 12, device=True), None), False, True),
    }


CALLS = ['save', 'restore', 'copy', 'expand', 'rollout', 'rollout_path_keys', 'rollout_rewards', 'playout', 'keys', 'successor_keys', 'sample_actions',
         'lidar_observation', 'agent_view', 'action_masks', 'walk_distances', 'walk_plans']


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('call', CALLS)
def test_skipped_pairs(world, call, layout):
    v, pool, spec = world
    run, has_dst, dense_ok = calls(world)[call]
    rs = np.random.RandomState(31)
    # (a restore moves at most num_envs rows: its list has 64 entries, one work-group, and the layouts are cut to it)
    cnt = N_ENVS if call == 'restore' else COUNT
    skip = {'third': np.r_[5, 17, 40:64], 'block': np.r_[3, 20:64]}[layout] if call == 'restore' else LAYOUTS[layout]
    live = np.setdiff1d(np.arange(cnt), skip)
    n_src = N_ENVS if call == 'save' else 2 * N_ENVS
    src = rs.randint(0, n_src, cnt).astype(np.int32)
    dst = rs.permutation(N_ENVS).astype(np.int32) if call == 'restore' else (200 + rs.permutation(cnt)).astype(np.int32)
    # the skipped pairs: the source, the destination, or both are NONE
    s_none, d_none = src.copy(), dst.copy()
    for i, j in enumerate(skip):
        if not has_dst or i % 3 != 1:
            s_none[j] = IDX_NONE
        if has_dst and i % 3 != 0:
            d_none[j] = IDX_NONE
    bad = np.where(s_none == IDX_NONE, -1, s_none).astype(np.int32), np.where(d_none == IDX_NONE, -1, d_none).astype(np.int32)
    if has_dst and call != 'restore':                      # the destination slots blank again (slots 380 .. were never written)
        pool.copy(np.arange(380, 380 + COUNT), np.arange(200, 200 + COUNT))
    v.sync()
    before = v.get_state() if call == 'restore' else pool.state()
    assert v.error_flags() == 0

    got, rows = run(s_none, d_none)
    v.sync()
    assert not v.error_flags() & F_BAD_INDEX, "a skipped pair raised F_BAD_INDEX"
    got = leaves(got)
    # destination rows named by no live pair: byte-identical
    if rows is not None:
        named = dst[live]
        untouched = np.setdiff1d(np.arange(len(before['map'])), named)
        for k in before:
            assert np.asarray(rows[k])[untouched].tobytes() == np.asarray(before[k])[untouched].tobytes(), (call, k)
        if call != 'restore':
            assert any(np.asarray(rows[k])[named].tobytes() != np.asarray(before[k])[named].tobytes() for k in before), "the live pairs wrote nothing"

    # the same pairs with a bad index in the place of NONE: the same outputs everywhere, and the flag
    exp, rows_bad = run(*bad)
    v.sync()
    assert v.error_flags() & F_BAD_INDEX
    for a, b in zip(got, leaves(exp)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), call
    if rows is not None:
        for k in rows:
            assert np.asarray(rows[k]).tobytes() == np.asarray(rows_bad[k]).tobytes(), (call, k)

    # the same pairs with a valid index in the place of NONE: the live rows at equal pair numbers
    if call != 'restore':
        s_fill = np.where(s_none == IDX_NONE, 0, s_none).astype(np.int32)
        d_fill = np.where(d_none == IDX_NONE, dst, d_none).astype(np.int32)
        filled, _ = run(s_fill, d_fill)
        for a, b in zip(got, leaves(filled)):
            ax = pair_axis(a, COUNT)
            assert np.take(a, live, ax).tobytes() == np.take(b, live, ax).tobytes(), call
        # ... and the dense call on the live entries alone
        if dense_ok and got:
            dense, _ = _dense(world, call, s_none, d_none, live)
            for a, b in zip(got, leaves(dense)):
                ax = pair_axis(a, COUNT)
                assert np.take(a, live, ax).tobytes() == b.tobytes(), call
    v.sync()
    assert v.error_flags() == 0

    # one -1 among them still raises the flag
    s_one = s_none.copy()
    s_one[live[1]] = -1
    run(s_one, d_none)
    v.sync()
    assert v.error_flags() & F_BAD_INDEX


def _dense(world, call, src, dst, live):
    """The call on the live entries alone, with each live pair's own per-pair inputs."""
    import torch
    v, pool, spec = world
    A, K = len(spec.actions_id), len(spec.items_id)
    rs = np.random.RandomState(9)
    acts = rs.randint(0, A, 4 * COUNT).astype(np.int32)
    items = rs.randint(0, K, 4 * COUNT).astype(np.int32)
    s, d = dev(src[live]), dev(dst[live])
    plans = dev(np.ascontiguousarray(acts.reshape(4, -1)[:, :COUNT][:, live]))
    if call in ('save', 'copy'):
        return None, None
    if call == 'expand':
        return pool.expand(s, dev(acts[:COUNT][live]), d, device=True), None
    if call == 'rollout':
        return pool.rollout(s, plans, d, device=True), None
    if call == 'rollout_path_keys':
        return pool.rollout(s, plans, d, device=True, path_keys=True), None
    if call == 'rollout_rewards':
        return pool.rollout(s, plans, None, device=True, rewards=True, observe='lidar'), None
    if call == 'walk_plans':
        return pool.walk_plans(s, dev(items[:COUNT][live]), 12, device=True), None
    return getattr(pool, call)(s, device=True), None


# ---------------------------------------------------------------------------------------------------------------- the closed loop
def bfs_host(v, pool, table, roots, depth, limit):
    """Breadth-first search the existing way: fresh_pairs and host-chosen slots, one round trip per iteration."""
    import torch
    parents = dev(np.arange(roots))
    pool.insert_keys(table, parents, device=True)
    cursor = roots
    for _ in range(depth):
        succ, found = pool.insert_successor_keys(table, parents, device=True)
        p, a = fresh_pairs(found.fresh)
        assert int(p.numel()) <= 4096, "the search outgrew the frontier this test gives the device loop"
        n = min(int(p.numel()), limit - cursor)
        children = torch.arange(cursor, cursor + n, dtype=torch.int32, device='cuda')
        if n:
            pool.expand(parents[p[:n]].contiguous(), a[:n].to(torch.int32).contiguous(), children, device=True)
        cursor += n
        parents = children
        if n == 0:
            break
    v.sync()
    return cursor


def bfs_device(v, pool, table, roots, depth, limit, capacity):
    """... and with a Frontier at fixed capacity: nothing in the loop waits for the host."""
    fr = pool.frontier(capacity)
    fr.reset_cursor(roots)
    parents = dev(np.r_[np.arange(roots), np.full(capacity - roots, IDX_NONE)])
    pool.insert_keys(table, parents, device=True)
    for _ in range(depth):
        succ, found = pool.insert_successor_keys(table, parents, device=True)
        p, a = fr.fresh_pairs(found.fresh, parents)
        c = fr.alloc(limit)
        pool.expand(p, a, c, device=True)
        parents = c.clone()
    v.sync()
    return int(host(fr.cursor)[0])


@pytest.mark.parametrize('limit', [None, 'third iteration'])
def test_closed_loop_breadth_first_search(world, limit):
    """4 iterations from 8 saved roots, both ways: the pool's rows, the cursor and the table's size agree.  With a limit that the third
    iteration reaches: the flag, no slot beyond the limit written, the rows below it the host loop's."""
    v, _, spec = world
    roots, depth, cap_pool, capacity = 8, 4, 8192, 4096
    if limit is not None:
        # where the host loop stands after 2 and after 3 iterations: a limit strictly between
        probe, t = v.snapshot(cap_pool), v.key_table(1 << 14)
        probe.save(envs=np.arange(roots), slots=np.arange(roots))
        after2 = bfs_host(v, probe, t, roots, 2, cap_pool)
        t.clear()
        after3 = bfs_host(v, probe, t, roots, 3, cap_pool)
        probe.close(); t.close()
        assert after3 > after2 + 1
        limit_n = (after2 + after3) // 2
    else:
        limit_n = cap_pool
    out = {}
    for way in ('host', 'device'):
        pool, table = v.snapshot(cap_pool), v.key_table(1 << 14)
        pool.save(envs=np.arange(roots), slots=np.arange(roots))
        v.sync()
        blank = pool.state()
        if way == 'host':
            cursor = bfs_host(v, pool, table, roots, depth, limit_n)
            assert v.error_flags() == 0
        else:
            cursor = bfs_device(v, pool, table, roots, depth, limit_n, capacity)
            assert v.error_flags() == (0 if limit is None else F_FRONTIER_FULL)
        out[way] = (cursor, pool.state(), len(table), blank)
        pool.close(); table.close()
    (c_h, rows_h, len_h, blank), (c_d, rows_d, len_d, _) = out['host'], out['device']
    assert c_h == c_d and c_d <= limit_n and (limit is None or c_d == limit_n) and c_d > roots
    for k in rows_h:
        assert np.asarray(rows_h[k])[:c_d].tobytes() == np.asarray(rows_d[k])[:c_d].tobytes(), k
        assert np.asarray(rows_d[k])[c_d:].tobytes() == np.asarray(blank[k])[c_d:].tobytes(), "a slot beyond the cursor was written: %s" % k
    if limit is None:
        assert len_h == len_d
