"""Search runs without a GPU (gym_novel_gridworlds_amd/search.py; include/ngw.h ngw_search_*): relax_reference - the numpy statement of the
offer, judge and settle steps around the table and the frontier - against a brute-force statement in plain loops on random small inputs
(padded parents, parents outside the pool, duplicate keys, refused keys, the overflow edge, goals and deaths); the model of
tests/search_oracle.py against tests/key_value_oracle.label_correcting for the synthetic costs; the host-side checks; header and binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import expand_oracle as XO
import frontier_oracle as FO
import key_value_oracle as KV
import ngw_testlib as T
import search_oracle as SX
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import _cabi, search as S
from gym_novel_gridworlds_amd.key_table import TAG_ROOT, VALUE_NONE
from gym_novel_gridworlds_amd.spec import IDX_NONE, STEP_COSTS, make_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN = -(1 << 31)


def brute_force(parents, g, bucket, info, keys, where, model, cursor, A, lut, by_action, keep, stop, goal, limit):
    """One iteration between successor keys and expand, position by position; g and bucket (lists) and the model are updated in place."""
    cap, pool = len(parents), len(g)
    n = cap * A
    values, tags, overflow = [VALUE_NONE] * n, [TAG_ROOT] * n, 0
    for q in range(n):
        j, a = divmod(q, A)
        p = int(parents[j])
        if not 0 <= p < pool or g[p] == VALUE_NONE:
            continue
        total = g[p] + int(lut[a if by_action else (int(info[q]) >> 2) & 63])
        if total >= VALUE_NONE or total < I32_MIN:
            overflow += 1
            continue
        values[q], tags[q] = total, bucket[p] * A + a
    refused = [int(where[q]) < 0 and int(keys[q]) != 0 for q in range(n)]
    _, _, best = model.insert_min(keys, values, tags, refused)
    improved = int(best.sum())
    best = best.copy()
    for q in range(n):
        if not best[q]:
            continue
        w = int(info[q])
        if (w >> 1) & 1 and (w >> 8) & 255 != 14:
            goal = min(goal, (values[q], int(where[q])))                              # (buckets are not negative where best is set)
        if stop and (w >> 1) & 1:
            best[q] = False
    if keep is None:
        first, second, count, full = FO.compact(best, A, None, cap)
    else:
        first, second, count = SX.select(values, best, keep, A, cap)
        full = False
    slots, cursor, short = FO.alloc(count[0], cursor, limit, cap)
    plist, nxt, expanded = [IDX_NONE] * cap, [IDX_NONE] * cap, 0
    for k in range(cap):
        j, a, c = int(first[k]), int(second[k]), int(slots[k])
        if j == IDX_NONE:
            continue
        plist[k] = int(parents[j])
        if c != IDX_NONE:
            g[c], bucket[c], nxt[k] = values[j * A + a], int(where[j * A + a]), c
            expanded += 1
    return dict(values=values, tags=tags, best=best, goal=goal, parents=plist, actions=list(second), children=list(slots), next_parents=nxt,
                cursor=cursor, offered=sum(v != VALUE_NONE for v in values), improved=improved, expanded=expanded, overflow=overflow,
                full=bool(full or short))


@pytest.mark.parametrize('seed', range(12))
def test_relax_reference_against_a_brute_force_statement(seed):
    rs = np.random.RandomState(seed)
    cap, A, pool = int(rs.randint(1, 9)), int(rs.randint(1, 5)), 12
    n = cap * A
    by_action = bool(seed & 1)
    keep = [None, None, 0, 2, cap][seed % 5]
    stop = bool(seed & 2)
    lut = np.zeros(64, np.int32)
    lut[:22] = rs.randint(0, 50, 22)
    model, held, goal = KV.KeyValueModel(), {}, (VALUE_NONE, -1)
    g = [VALUE_NONE] * pool
    bucket = [-1] * pool
    for s in range(pool // 2):                                                         # slots reached earlier, two of them at the overflow edge
        g[s], bucket[s] = int(rs.randint(0, 30)), int(rs.randint(0, 64))
    g[0], g[1] = VALUE_NONE - 10, VALUE_NONE - 1
    lut[0], lut[1] = 9, 10                                                             # (VALUE_NONE - 10) + 9 is the last value that is one
    cursor, limit = int(rs.randint(0, pool)), pool
    bucket_of = {}
    for it in range(4):
        parents = rs.randint(0, pool, cap)
        parents[rs.rand(cap) < 0.25] = IDX_NONE                                        # padded
        parents[rs.rand(cap) < 0.1] = pool + 3                                         # outside the pool
        parents[rs.rand(cap) < 0.3] = rs.randint(0, 2)                                 # the overflow edge
        keys = rs.randint(0, 7, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)   # duplicates, and key 0
        for k in set(keys.tolist()) - {0}:
            bucket_of.setdefault(k, len(bucket_of))
        where = np.array([bucket_of[k] if k and k % 5 != 3 else -1 for k in keys.tolist()], np.int32)    # (some keys the table refuses)
        code, msg = rs.randint(0, 22, n), np.where(rs.rand(n) < 0.3, 14, rs.randint(0, 14, n))
        info = (rs.randint(0, 2, n) | ((rs.rand(n) < 0.4).astype(np.int64) << 1) | (code << 2) | (msg << 8)).astype(np.uint32)
        g_np, bucket_np = np.array(g, np.int32), np.array(bucket, np.int32)
        e = brute_force(parents, g, bucket, info, keys, where, model, cursor, A, lut, by_action, keep, stop, goal, limit)
        r = S.relax_reference(parents.astype(np.int32), g_np, bucket_np, info, keys, where, held, cursor, A, lut, by_action, keep, stop,
                              S.SearchGoal(*goal), limit)
        for name in ('values', 'tags', 'best', 'parents', 'actions', 'children', 'next_parents'):
            assert np.asarray(getattr(r, name)).tolist() == np.asarray(e[name]).tolist(), (it, name)
        for name in ('cursor', 'offered', 'improved', 'expanded', 'overflow', 'full'):
            assert getattr(r, name) == e[name], (it, name)
        assert tuple(r.goal) == e['goal'] and g_np.tolist() == g and bucket_np.tolist() == bucket
        assert {k: list(v) for k, v in held.items()} == {k: list(v) for k, v in model.held.items()}
        cursor, goal = e['cursor'], e['goal']
        g, bucket = g_np.tolist(), bucket_np.tolist()
    # the inputs did what they were made for
    assert isinstance(r, S.Relaxed)


def test_the_overflow_edge_of_the_offer():
    """g + cost == VALUE_NONE - 1 is the last offer; VALUE_NONE itself and everything beyond is none, is counted, and never wraps."""
    lut = np.zeros(64, np.int32)
    lut[:4] = [9, 10, 11, (1 << 31) - 2]
    g = np.array([VALUE_NONE - 10, VALUE_NONE, 5], np.int32)
    bucket = np.array([7, 8, 9], np.int32)
    parents = np.array([0, 1, 2, IDX_NONE, 3, -1], np.int32)
    values, tags, over = S.offer_reference(parents, g, bucket, np.zeros(24, np.uint32), 4, lut, True)
    assert values.reshape(6, 4).tolist() == [[VALUE_NONE - 1, VALUE_NONE, VALUE_NONE, VALUE_NONE], [VALUE_NONE] * 4,
                                             [14, 15, 16, VALUE_NONE]] + [[VALUE_NONE] * 4] * 3
    assert tags.reshape(6, 4).tolist() == [[28, -1, -1, -1], [-1] * 4, [36, 37, 38, -1]] + [[-1] * 4] * 3
    assert over.reshape(6, 4).tolist() == [[False, True, True, True], [False] * 4, [False, False, False, True]] + [[False] * 4] * 3
    negative = np.zeros(64, np.int32)
    negative[0] = -5
    values, _, over = S.offer_reference(np.array([0], np.int32), np.array([I32_MIN + 2], np.int32), np.array([0], np.int32), np.zeros(1, np.uint32), 1,
                                        negative, True)
    assert values.tolist() == [VALUE_NONE] and over.tolist() == [True]


def test_cost_tables():
    lut, by_action = S.cost_table(None, 1, 5)
    assert not by_action and lut.dtype == np.int32 and lut.shape == (64,)
    assert lut[:len(STEP_COSTS)].tolist() == [int(round(c)) for c in STEP_COSTS] == SX.step_cost_table() and not lut[len(STEP_COSTS):].any()
    assert S.cost_table(None, 100, 5)[0][2] == 2791 and S.cost_table(None, 100, 5)[0].tolist()[:22] == SX.step_cost_table(100)
    lut, by_action = S.cost_table([3, -1, 7], 1, 3)
    assert by_action and lut[:4].tolist() == [3, -1, 7, 0]
    for bad, what in (((None, 1 << 16, 5), 'scale'), ((None, -1, 5), 'scale'), (([1, 2], 1, 3), 'costs'), (([1.5, 2, 3], 1, 3), 'costs'),
                      (([1, 2, VALUE_NONE], 1, 3), 'costs')):
        with pytest.raises(ValueError, match=what):
            S.cost_table(*bad)


def test_roots_are_checked_on_the_host():
    r, n = S.check_roots([3, IDX_NONE, 0, 3], 4, 8)
    assert r.dtype == np.int32 and r.tolist() == [3, IDX_NONE, 0, 3] and n == 4
    assert S.check_roots([], 4, 8)[1] == 0
    for bad, what in (([4], 'outside'), ([-1], 'outside'), ([0.5], 'integer'), ([[1]], 'one-dimensional'), (None, 'expected'), (list(range(9)), 'capacity')):
        with pytest.raises(ValueError, match=what):
            S.check_roots(bad, 16 if what == 'capacity' else 4, 8)


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    assert int(re.search(r'#define NGW_SEARCH_ROWS (\d+)', text).group(1)) == _cabi.SEARCH_ROWS == S.STATS_ROWS
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    L = _cabi.lib()
    for name in ('ngw_search_create', 'ngw_search_destroy', 'ngw_search_start', 'ngw_search_run', 'ngw_search_read'):
        assert name in _cabi.SYMBOLS and getattr(L, name).argtypes, name
    assert L.ngw_abi_version() == 3
    assert C.sizeof(_cabi.SearchReport) == 40 + 16 * _cabi.SEARCH_ROWS and C.sizeof(_cabi.SearchArrays) == 5 * C.sizeof(C.c_void_p)
    # a NULL handle is refused before anything is touched
    assert L.ngw_search_run(None, None, 1, None) == _cabi.E_INVALID_ARG and L.ngw_search_read(None, None, None) == _cabi.E_INVALID_ARG


def test_the_model_against_the_label_correcting_oracle():
    """tests/search_oracle.py with the synthetic costs, frontier 256 and pool 512, beside key_value_oracle.label_correcting on the fixture of
    tests/test_key_values.py: the same keys, values and improved positions in every iteration, the same table, the same reopened count."""
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, 9)
    n, cap = 4, 256
    o = Oracle(spec.compile(), n, seed=XO.good_seed(spec, n))
    o.reset()
    A = spec.compile().n_actions
    costs = KV.synthetic_costs(spec)
    cpu = KV.label_correcting(spec, SO.oracle_state(o), costs, 4)
    m = SX.SearchModel(spec, cap, 512, costs=costs)
    m.save(SO.oracle_state(o), np.arange(n))
    m.cursor = n
    best = m.start(np.arange(n))
    model, e_keys, e_values, e_best = next(cpu)
    assert best.all() and m.parents[:n] == list(range(n)) and set(m.table.held) == set(model.held)
    for it in range(4):
        rec = m.iterate()
        model, e_keys, e_values, e_best = next(cpu)
        P = len(e_keys) // A
        assert (rec['keys'][:P * A] == e_keys).all() and not rec['keys'][P * A:].any()
        assert (rec['values'][:P * A] == e_values).all() and (rec['best'][:P * A] == e_best).all() and not rec['best'][P * A:].any()
        assert rec['improved'] == rec['expanded'] == int(e_best.sum()) and rec['offered'] == P * A and rec['overflow'] == 0
        assert {k: v[0] for k, v in m.table.held.items()} == {k: v[0] for k, v in model.held.items()}
    assert m.table.reopened == model.reopened >= n and not m.full and m.cursor == n + sum(r['improved'] for r in m.iterations)
    for k in list(model.held)[::7]:                                                    # the chains of the two models are the same plans
        assert KV.chain(m.table, k, costs) == KV.chain(model, k, costs)
