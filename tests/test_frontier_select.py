"""Priority frontiers on the MI355X (csrc/ngw_select.inc, include/ngw.h ngw_frontier_select, frontier.Frontier.select): both kernel forms against
frontier.select_reference byte for byte, the tie-break's determinism, the composition with alloc and the skipped pair, and a per-env beam search
and a global best-first search written with the selection on the device and with the reference on host copies."""
import ctypes as C
import itertools

import numpy as np
import pytest

import expand_oracle as XO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, frontier as F
from gym_novel_gridworlds_amd.key_table import VALUE_NONE, step_cost_values
from gym_novel_gridworlds_amd.spec import IDX_NONE, make_spec

pytestmark = pytest.mark.gpu
TILE = 4096                          # csrc/ngw_device.h NGW_FRONTIER_TILE
WAVE_MAX = F.SELECT_WAVE_MAX         # csrc/ngw_device.h NGW_SELECT_WAVE_MAX: the form changes behind it
N_ENVS = 64
E_INVALID_ARG = -1                   # include/ngw.h NGW_E_INVALID_ARG


def dev(x, dtype=np.int32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()
    torch.cuda.synchronize()
    return t


def host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


@pytest.fixture(scope='module')
def world():
    """One 10 x 10 Pogostick-v1 handle of 64 envs after 30 random steps; a pool of 512 slots whose first 128 hold the envs' states and a
    generation of children of them (the world of tests/test_frontier.py)."""
    spec = make_spec('NovelGridworld-Pogostick-v1', 10)
    v = VecNovelGridworld(spec=spec, num_envs=N_ENVS, seed=XO.good_seed(spec, N_ENVS), autoreset=True, horizon=40)
    v.reset()
    rs = np.random.RandomState(5)
    A = len(spec.actions_id)
    for _ in range(30):
        v.step(rs.randint(0, A, N_ENVS).astype(np.int32))
    pool = v.snapshot(512)
    pool.save(slots=np.arange(N_ENVS))
    pool.expand(rs.randint(0, N_ENVS, N_ENVS), rs.randint(0, A, N_ENVS), N_ENVS + np.arange(N_ENVS))
    v.sync()
    assert v.error_flags() == 0
    yield v, pool, spec
    v.close()


# ---------------------------------------------------------------------------------------------------------------- against the reference
PATTERNS = ('equal', 'two', 'range4', 'full', 'none')


def pattern(name, n, rs):
    if name == 'equal':
        return np.full(n, 7, np.int32)
    if name == 'two':
        return rs.choice(np.array([-3, 12], np.int32), n)
    if name == 'range4':
        return rs.randint(100, 104, n).astype(np.int32)
    if name == 'full':
        v = rs.randint(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
        if n:
            v[rs.randint(0, n, 3)] = np.array([-2 ** 31, 2 ** 31 - 2, VALUE_NONE], np.int32)
        return v
    return np.full(n, VALUE_NONE, np.int32)


def stray_flags(n, rs):
    f = (rs.randint(0, 3, n) != 0).astype(np.uint8)
    if n:
        f[rs.randint(0, n, 6)] = np.array([2, 0x80, 0xFF, 2, 0x80, 0xFF], np.uint8)      # any non-zero byte counts
    return f


def check(v, pool, values, vd, keep, div, amap, md, flags, fd, groups, largest, extra, where):
    import torch
    cap = groups * keep + extra
    fr = pool.frontier(cap)
    sel = fr.select(vd, keep, div, md, fd, groups, largest)
    e_first, e_second, e_taken, e_bound, e_count = F.select_reference(values, keep, div, amap, flags, groups, largest, cap)
    assert sel.first.dtype == sel.taken.dtype == sel.bound.dtype == torch.int32 and sel.first.shape == sel.second.shape == (cap,), where
    assert host(sel.first).tobytes() == e_first.tobytes(), where
    assert host(sel.second).tobytes() == e_second.tobytes(), where
    assert host(sel.taken).tobytes() == e_taken.tobytes() and host(sel.bound).tobytes() == e_bound.tobytes(), where
    assert host(fr.count_dev).tobytes() == e_count.tobytes(), where
    assert (host(sel.first)[groups * keep:] == IDX_NONE).all(), where
    assert v.error_flags() == 0, where
    fr.close()


SIZES = [0, 1, 15, 16, 17, 63, 64, 65, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
# what a call varies beside the values, the flags and keep: the tail behind the spans, div and map, the mode - every combination, taken in turn
VARIANTS = list(itertools.product((0, 70), ((1, False), (17, False), (17, True), (1, True)), (False, True)))


@pytest.mark.parametrize('m', SIZES)
def test_selection_against_the_reference(world, m):
    """Every pattern with and without flags and every keep around the largest group's candidates at every size and group count; the 16
    variants (tail, div, map, mode) taken in turn from call to call, so that the file stays at some 2 400 selections."""
    v, pool, _ = world
    turn = m                                                 # (a different start per size)
    for groups in ((1, 3, 65) if m <= WAVE_MAX else (1, 3)):
        n = groups * m
        rs = np.random.RandomState(1000 + 7 * m + groups)
        maps = {d: (rs.permutation(-(-n // d) + 3) + 7).astype(np.int32) for d in (1, 17)}
        maps_dev = {d: dev(a) for d, a in maps.items()}
        for name in PATTERNS:
            values = pattern(name, n, rs)
            vd = dev(values)
            for flags in (None, stray_flags(n, rs)):
                fd = None if flags is None else dev(flags, np.uint8)
                cand = (values != VALUE_NONE) & (True if flags is None else flags != 0)
                c = int(cand.reshape(groups, m).sum(1).max()) if n else 0
                for keep in sorted({0, 1, max(c - 1, 0), c, c + 5, c // 2}):
                    extra, (div, mapped), largest = VARIANTS[turn % len(VARIANTS)]
                    turn += 1
                    where = 'm %d groups %d %s flags %s keep %d div %d map %s largest %s extra %d' % (m, groups, name, flags is not None, keep, div, mapped,
                                                                                                     largest, extra)
                    check(v, pool, values, vd, keep, div, maps[div] if mapped else None, maps_dev[div] if mapped else None, flags, fd, groups, largest,
                          extra, where)


@pytest.mark.parametrize('m, groups', [(8 * 17, 8), (WAVE_MAX, 2), (TILE + 77, 1), (WAVE_MAX + 3, 3)])
def test_selection_without_second_and_misaligned_values(world, m, groups):
    """second_dev == NULL through the C-ABI, and a values pointer that is only 4-byte aligned (a slice from element 1), in both forms."""
    import torch
    v, pool, _ = world
    rs = np.random.RandomState(m)
    n, keep = m * groups, 9
    values = rs.randint(-50, 50, n + 1).astype(np.int32)
    values[rs.randint(0, n, 5)] = VALUE_NONE
    flags = stray_flags(n + 1, rs)
    vd, fd = dev(values), dev(flags, np.uint8)
    for off in (0, 1):
        val, flg = values[off:off + n], flags[off:off + n]
        cap = groups * keep + 5
        e = F.select_reference(val, keep, 17, None, flg, groups, False, cap)
        first = torch.full((cap,), 123, dtype=torch.int32, device='cuda')
        taken = torch.full((groups,), 123, dtype=torch.int32, device='cuda')
        bound = torch.full((groups,), 123, dtype=torch.int32, device='cuda')
        count = torch.full((2,), 123, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        rc = _cabi.lib().ngw_frontier_select(v._h, C.c_void_p(vd.data_ptr() + 4 * off), C.c_void_p(fd.data_ptr() + off), n, groups, 17, None, keep, 0, cap,
                                             C.c_void_p(first.data_ptr()), None, C.c_void_p(taken.data_ptr()), C.c_void_p(bound.data_ptr()),
                                             C.c_void_p(count.data_ptr()))
        assert rc == 0
        v.sync()
        assert (host(first) == e[0]).all() and (host(taken) == e[2]).all() and (host(bound) == e[3]).all() and (host(count) == e[4]).all()
        fr = pool.frontier(cap)
        sel = fr.select(vd[off:off + n], keep, 17, None, fd[off:off + n], groups)
        assert (host(sel.first) == e[0]).all() and (host(sel.second) == e[1]).all() and (host(sel.taken) == e[2]).all()
        fr.close()
    assert v.error_flags() == 0


@pytest.mark.parametrize('m, groups', [(3 * TILE + 5, 1), (1000, 65)])
def test_the_same_input_twice_gives_the_same_bytes(world, m, groups):
    """All values equal: only the position decides."""
    v, pool, _ = world
    n = m * groups
    values = np.full(n, -4, np.int32)
    rs = np.random.RandomState(m)
    flags = stray_flags(n, rs)
    keep = m // 3
    out = []
    for _ in range(2):
        fr = pool.frontier(groups * keep + 3)
        sel = fr.select(dev(values), keep, 17, None, dev(flags, np.uint8), groups, True)
        out.append([host(x).tobytes() for x in (sel.first, sel.second, sel.taken, sel.bound, fr.count_dev)])
    assert out[0] == out[1]
    e = F.select_reference(values, keep, 17, None, flags, groups, True, groups * keep + 3)
    assert out[0] == [x.tobytes() for x in e]
    assert v.error_flags() == 0


def test_python_argument_checks(world):
    import torch
    v, pool, _ = world
    fr = pool.frontier(8)
    ok = torch.arange(12, dtype=torch.int32, device='cuda')
    for bad in (np.arange(12, dtype=np.int32), ok.long(), ok.cpu(), ok[::2]):
        with pytest.raises(ValueError, match='values'):
            fr.select(bad, 2)
    with pytest.raises(ValueError, match='keep'):
        fr.select(ok, 3, groups=3)                       # 9 entries in a list of 8
    with pytest.raises(ValueError, match='groups'):
        fr.select(ok, 1, groups=5)
    with pytest.raises(ValueError, match='div'):
        fr.select(ok, 1, div=0)
    with pytest.raises(ValueError, match='flags'):
        fr.select(ok, 1, flags=torch.ones(11, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='map'):
        fr.select(ok, 1, div=3, map=torch.zeros(3, dtype=torch.int32, device='cuda'))
    fr.close()
    with pytest.raises(ValueError, match='closed'):
        fr.select(ok, 1)
    assert v.error_flags() == 0


def test_validation_through_the_c_abi(world):
    """Each is refused with NGW_E_INVALID_ARG before anything is launched: the outputs keep their bytes."""
    import torch
    v, _, _ = world
    L = _cabi.lib()
    values = torch.arange(64, dtype=torch.int32, device='cuda')
    first, second = torch.full((16,), 5, dtype=torch.int32, device='cuda'), torch.full((16,), 5, dtype=torch.int32, device='cuda')
    taken, bound, count = (torch.full((2,), 5, dtype=torch.int32, device='cuda') for _ in range(3))
    torch.cuda.synchronize()

    def call(values_ptr=values.data_ptr(), n=64, groups=2, div=1, keep=8, largest=0, capacity=16):
        return L.ngw_frontier_select(v._h, C.c_void_p(values_ptr) if values_ptr else None, None, n, groups, div, None, keep, largest, capacity,
                                     C.c_void_p(first.data_ptr()), C.c_void_p(second.data_ptr()), C.c_void_p(taken.data_ptr()), C.c_void_p(bound.data_ptr()),
                                     C.c_void_p(count.data_ptr()))
    assert call(keep=-1) == E_INVALID_ARG
    assert call(keep=9) == E_INVALID_ARG                        # groups * keep > capacity
    assert call(n=(1 << 24) + 2) == E_INVALID_ARG
    assert call(div=0) == E_INVALID_ARG
    assert call(values_ptr=0) == E_INVALID_ARG                   # NULL values with n > 0
    assert call(groups=0) == E_INVALID_ARG and call(groups=3) == E_INVALID_ARG and call(largest=2) == E_INVALID_ARG
    v.sync()
    for x in (first, second, taken, bound, count):
        assert (host(x) == 5).all()
    assert call() == 0
    v.sync()
    assert host(taken).tolist() == [8, 8] and host(bound).tolist() == [7, 39] and host(count).tolist() == [16, 64]
    assert v.error_flags() == 0


# ---------------------------------------------------------------------------------------------------------------- with alloc and the skipped pair
def test_one_group_allocates_exactly_the_taken(world):
    v, pool, _ = world
    rs = np.random.RandomState(8)
    values = rs.randint(0, 9, 300).astype(np.int32)
    flags = (rs.randint(0, 4, 300) == 0).astype(np.uint8)
    total = int(flags.sum())
    for keep in (10, total + 4):
        fr = pool.frontier(total + 10)
        fr.reset_cursor(40)
        sel = fr.select(dev(values), keep, flags=dev(flags, np.uint8))
        slots = host(fr.alloc())
        taken = min(keep, total)
        assert int(host(sel.taken)[0]) == taken == fr.count() and fr.total() == total
        assert (slots[:taken] == 40 + np.arange(taken)).all() and (slots[taken:] == IDX_NONE).all() and int(host(fr.cursor)[0]) == 40 + taken
        fr.close()
    assert v.error_flags() == 0


def test_several_groups_expand_the_live_entries_and_skip_the_padding(world):
    """Three groups of 8 parents, keep 6, the middle group with two candidates only: alloc() serves all 18 entries, the expand through the
    lists writes exactly the live children - as the same expand of the live entries alone does - and leaves the padded entries' slots alone."""
    v, pool, spec = world
    A = len(spec.actions_id)
    rs = np.random.RandomState(21)
    groups, rows, keep = 3, 8, 6
    parents = rs.permutation(128)[:groups * rows].astype(np.int32)
    values = rs.randint(0, 5, (groups * rows, A)).astype(np.int32)
    flags = (rs.randint(0, 3, (groups * rows, A)) == 0).astype(np.uint8)
    flags[rows:2 * rows] = 0
    flags[rows + 2, 3] = flags[rows + 5, 0] = 0x80
    e_first, e_second, e_taken, _, e_count = F.select_reference(values, keep, A, parents, flags, groups, False, groups * keep + 4)
    assert e_taken.tolist() == [6, 2, 6]
    fr = pool.frontier(groups * keep + 4)
    fr.reset_cursor(200)
    p, a = fr.best_pairs(dev(values), dev(parents), keep, groups, dev(flags, np.uint8))
    c = fr.alloc()
    assert (host(p) == e_first).all() and (host(a) == e_second).all() and (host(fr.count_dev) == e_count).all() and fr.count() == groups * keep
    assert (host(c) == np.r_[200 + np.arange(groups * keep), [IDX_NONE] * 4]).all()
    pool.copy(np.arange(380, 380 + 32), np.arange(200, 200 + 32))            # (slots 380 .. were never written: the destinations blank)
    v.sync()
    blank = pool.state()
    pool.expand(p, a, c, device=True)
    v.sync()
    padded = pool.state()
    live = np.flatnonzero(e_first != IDX_NONE)
    assert len(live) == 14
    pool.copy(np.arange(380, 380 + 32), np.arange(200, 200 + 32))
    pool.expand(dev(e_first[live]), dev(e_second[live]), dev(200 + live), device=True)
    v.sync()
    dense = pool.state()
    skipped = 200 + np.setdiff1d(np.arange(32), live)
    for k in blank:
        assert np.asarray(padded[k]).tobytes() == np.asarray(dense[k]).tobytes(), k
        assert np.asarray(padded[k])[skipped].tobytes() == np.asarray(blank[k])[skipped].tobytes(), k
    assert any(np.asarray(padded[k])[200 + live].tobytes() != np.asarray(blank[k])[200 + live].tobytes() for k in blank), "the live pairs wrote nothing"
    assert v.error_flags() == 0
    fr.close()


# ---------------------------------------------------------------------------------------------------------------- the closed loops
def beam_search(v, spec, way, B=4, depth=4):
    """A beam of B states per env in fixed slots: generation t of env e in slots (t % 2) * 256 + e * B + i.  way 'device': nothing in the loop
    waits for the host; 'host': the same calls, the lists from select_reference on host copies."""
    import torch
    A = len(spec.actions_id)
    n_slots = N_ENVS * B
    pool = v.snapshot(2 * n_slots)
    fr = pool.frontier(n_slots)
    pool.save(envs=np.arange(N_ENVS), slots=np.arange(N_ENVS) * B)
    beam = dev(np.where(np.arange(n_slots) % B == 0, np.arange(n_slots), IDX_NONE))
    g = torch.full((2 * n_slots + 1,), VALUE_NONE, dtype=torch.int32, device='cuda')             # (one more entry: where padded entries write)
    g[(torch.arange(N_ENVS, device='cuda') * B).long()] = 0
    lists = []
    for it in range(depth):
        base, other = (it % 2) * n_slots, ((it + 1) % 2) * n_slots
        succ = pool.successor_keys(beam, device=True)
        live, pi = (beam != IDX_NONE)[:, None], beam.clamp(min=0).long()
        values = torch.where(live, g[pi][:, None] + step_cost_values(succ.info, 1), VALUE_NONE).to(torch.int32).contiguous()
        if way == 'device':
            sel = fr.select(values, B, A, beam, None, N_ENVS)
            first, second, taken, bound = sel
        else:
            e = F.select_reference(host(values), B, A, host(beam), None, N_ENVS, False, n_slots)
            first, second, taken, bound = (dev(x) for x in e[:4])
        children = torch.arange(other, other + n_slots, dtype=torch.int32, device='cuda')
        pool.expand(first, second, children, device=True)
        chosen = first != IDX_NONE
        pos = (first - base).clamp(min=0).long() * A + second.clamp(min=0).long()                 # (the beam's slots are base + its rows)
        at = torch.where(chosen, children, 2 * n_slots).long()
        g[at] = torch.where(chosen, values.reshape(-1)[pos], VALUE_NONE)
        g[2 * n_slots] = VALUE_NONE
        beam = torch.where(chosen, children, IDX_NONE).to(torch.int32).contiguous()
        lists.append((first.clone(), second.clone(), taken.clone(), bound.clone()))
    v.sync()
    out = ([[host(x) for x in l] for l in lists], host(g), pool.keys(np.arange(2 * n_slots)))
    assert v.error_flags() == 0
    fr.close()
    pool.close()
    return out


def test_per_env_beam_search_both_ways(world):
    v, _, spec = world
    A = len(spec.actions_id)
    assert 4 * A <= WAVE_MAX                                     # the wave form
    (l_d, g_d, k_d), (l_h, g_h, k_h) = beam_search(v, spec, 'device'), beam_search(v, spec, 'host')
    for it, (a, b) in enumerate(zip(l_d, l_h)):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), "iteration %d" % it
    assert g_d.tobytes() == g_h.tobytes() and k_d.tobytes() == k_h.tobytes()
    assert all((l[2] > 0).all() for l in l_d) and (l_d[-1][2] == 4).all(), "the beams did not fill up"
    assert (g_d != VALUE_NONE).sum() > 2 * N_ENVS


def best_first(v, spec, way, keep=32, iterations=4, roots=32, capacity=128, cap_pool=1024):
    """One pool, one valued key table, one group: successor_keys -> insert_min -> select(best) -> alloc -> expand.  The parents are padded to
    the frontier's capacity, so n = capacity * A values: the grid form."""
    import torch
    A = len(spec.actions_id)
    assert capacity * A > WAVE_MAX
    pool, table = v.snapshot(cap_pool), v.key_table(8192, values=True)
    fr = pool.frontier(capacity)
    pool.save(envs=np.arange(roots), slots=np.arange(roots))
    fr.reset_cursor(roots)
    parents = dev(np.r_[np.arange(roots), np.full(capacity - roots, IDX_NONE)])
    arange_a = dev(np.arange(A))
    g = torch.full((cap_pool + 1,), VALUE_NONE, dtype=torch.int32, device='cuda')
    g[:roots] = 0
    keys, _ = pool.insert_keys_min(table, parents, torch.zeros(capacity, dtype=torch.int32, device='cuda'), device=True)
    lists, seen = [], [keys.clone()]
    for it in range(iterations):
        succ = pool.successor_keys(parents, device=True)
        live, pi = (parents != IDX_NONE)[:, None], parents.clamp(min=0).long()
        g_child = torch.where(live, g[pi][:, None] + step_cost_values(succ.info, 1), VALUE_NONE).to(torch.int32).contiguous()
        tags = (pi[:, None] * A + arange_a[None, :]).to(torch.int32).contiguous()                 # parent slot * A + action
        found = table.insert_min(succ.keys.reshape(-1), g_child.reshape(-1), tags=tags.reshape(-1), device=True)
        if way == 'device':
            sel = fr.select(g_child, keep, A, parents, found.best)
            first, second, taken, bound = sel
        else:
            e = F.select_reference(host(g_child), keep, A, host(parents), host(found.best).astype(np.uint8), 1, False, capacity)
            first, second, taken, bound = (dev(x) for x in e[:4])
            fr.count_dev.copy_(dev(e[4]))                                                         # (what alloc reads)
        c = fr.alloc()
        pool.expand(first, second, c, device=True)
        value = table.read(table.lookup(pool.keys(c, device=True), device=True), device=True)[0]  # a chosen child's offer is what the table holds
        g[torch.where(c != IDX_NONE, c, cap_pool).long()] = value
        g[cap_pool] = VALUE_NONE
        lists.append((first.clone(), second.clone(), taken.clone(), bound.clone(), c.clone(), fr.count_dev.clone()))
        seen.append(succ.keys.reshape(-1).clone())
        parents = c.clone()
    v.sync()
    ks = np.unique(np.concatenate([host(s).view(np.uint64) for s in seen]))
    ks = ks[ks != 0]
    stored = table.lookup(ks) >= 0
    value, tag = table.get(ks[stored])
    out = ([[host(x) for x in l] for l in lists], len(table), ks[stored], np.asarray(value), np.asarray(tag), int(host(fr.cursor)[0]))
    assert v.error_flags() == 0
    for x in (fr, pool, table):
        x.close()
    return out


def test_global_best_first_both_ways(world):
    v, _, spec = world
    d, h = best_first(v, spec, 'device'), best_first(v, spec, 'host')
    for it, (a, b) in enumerate(zip(d[0], h[0])):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), "iteration %d" % it
    assert d[1] == h[1] and d[5] == h[5] and d[5] > 32
    assert d[2].tobytes() == h[2].tobytes() and d[3].tobytes() == h[3].tobytes() and d[4].tobytes() == h[4].tobytes()
    assert any(int(l[5][1]) > 32 and int(l[2][0]) == 32 for l in d[0]), "never more improved children than keep: the cut was not exercised"
