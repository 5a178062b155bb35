"""Open-list search runs without a GPU (gym_novel_gridworlds_amd/search.py open_list=True; include/ngw.h "an open-list iteration"):
walk_heuristic_reference against a brute-force statement; take_reference / open_reference / best_first_reference against a brute-force
open list - a Python dict of slot -> f, choosing the `keep` smallest (f, slot) - on random small inputs; the model of
tests/best_first_oracle.py against key_value_oracle.label_correcting (choosing the whole open list IS the layered search), on a scenario
that supersedes, and on the goal state of tests/test_search_run.py with and without the walk heuristic; header and binding."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import best_first_oracle as BF
import expand_oracle as XO
import key_value_oracle as KV
import ngw_testlib as T
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import _cabi, search as S
from gym_novel_gridworlds_amd.key_table import VALUE_NONE
from gym_novel_gridworlds_amd.spec import ACT_LEFT, ACT_RIGHT, IDX_NONE, STEP_COSTS, make_spec
from test_search_run import goal_state
from test_search_run_cpu import brute_force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, CAP_POOL = 256, 512


def oracle_env(state_of=None):
    """The 9 x 9 Pogostick fixture of tests/test_search_run.py on the CPU oracle -> (spec, the four states)."""
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, 9)
    o = Oracle(spec.compile(), 4, seed=XO.good_seed(spec, 4))
    o.reset()
    st = SO.oracle_state(o)
    if state_of is not None:
        st = state_of(types.SimpleNamespace(map_size=9, spec=spec, num_envs=4, get_state=lambda: st))
    return spec, st


def model_of(spec, st, keep, n_roots=None, **kw):
    m = BF.BestFirstModel(spec, CAP, CAP_POOL, keep, **kw)
    m.save(st, np.arange(4))
    m.cursor = 4
    m.start(np.arange(4 if n_roots is None else n_roots))
    return m


# ------------------------------------------------------------------ the heuristic
def brute_h(dist, weights, mode):
    terms = [int(w) * int(d) for w, d in zip(weights, dist) if w > 0 and d >= 0]
    return min((min if mode == 'min' else max)(terms), VALUE_NONE - 1) if terms else 0


@pytest.mark.parametrize('mode', ['min', 'max'])
def test_walk_heuristic_reference_against_a_brute_force_statement(mode):
    rs = np.random.RandomState(3)
    for K in (1, 2, 3, 4, 7, 8, 13):
        dist = rs.randint(-1, 40, (50, K)).astype(np.int32)
        weights = np.where(rs.rand(K) < 0.4, 0, rs.randint(1, 1000, K)).astype(np.int32)
        dist[0], dist[1] = -1, 0                                                       # nothing reachable; everything faced already
        got = S.walk_heuristic_reference(dist, weights, mode)
        assert got.dtype == np.int32 and got.tolist() == [brute_h(d, weights, mode) for d in dist], (K, mode)
        assert got[0] == 0
        assert S.walk_heuristic_reference(dist, np.zeros(K, np.int32), mode).tolist() == [0] * 50       # weights 0: no term anywhere
        assert int(S.walk_heuristic_reference(dist[5], weights, mode)) == brute_h(dist[5], weights, mode)  # one row
    # the product is taken in 64 bits and clamped: 2^30 * 4 = 2^32 would wrap an int32 to 0
    big = np.array([1 << 30, 3], np.int32)
    assert S.walk_heuristic_reference(np.array([[4, 5]], np.int32), big, mode).tolist() == [15 if mode == 'min' else VALUE_NONE - 1]
    assert S.walk_heuristic_reference(np.array([[4, -1]], np.int32), big, mode).tolist() == [VALUE_NONE - 1]
    assert BF.heuristic_of([4, -1], big, mode) == VALUE_NONE - 1
    with pytest.raises(ValueError, match='mode'):
        S.walk_heuristic_reference(np.zeros((1, 2), np.int32), big, 'mean')


def test_priority_saturates_below_value_none():
    g = np.array([VALUE_NONE - 3, 5, -(1 << 31), VALUE_NONE - 1], np.int32)
    h = np.array([VALUE_NONE - 1, 7, 0, 0], np.int32)
    assert S.priority_reference(g, h).tolist() == [VALUE_NONE - 1, 12, -(1 << 31), VALUE_NONE - 1]


def test_heuristics_are_checked_on_the_host():
    mode, w = S.check_heuristic(S.WalkHeuristic([0, 3, 5], 'max'), 3)
    assert mode == _cabi.SEARCH_H_MAX and w.dtype == np.int32 and w.tolist() == [0, 3, 5]
    assert S.check_heuristic(None, 3) == (_cabi.SEARCH_H_NONE, None)
    for bad, what in ((S.WalkHeuristic([0, -1, 5], 'min'), 'weights'), (S.WalkHeuristic([0, 1], 'min'), 'weights'), (S.WalkHeuristic([0.5, 1, 2], 'min'), 'weights'),
                      (S.WalkHeuristic([0, 1, 2], 'mean'), 'mode'), ('min', 'WalkHeuristic')):
        with pytest.raises(ValueError, match=what):
            S.check_heuristic(bad, 3)


# ------------------------------------------------------------------ the references against a brute-force open list
def random_open_list(seed):
    """Four iterations on random inputs: the open list as a dict slot -> f, the `keep` smallest (f, slot) chosen; steps 2 to 6 from the
    brute-force statement of tests/test_search_run_cpu.py with the compaction; superseding and opening in plain loops."""
    rs = np.random.RandomState(100 + seed)
    cap, A, pool, K, n_buckets = int(rs.randint(2, 9)), int(rs.randint(1, 5)), 16, int(rs.randint(1, 6)), 8
    n = cap * A
    keep, by_action, stop, prune = int(rs.randint(1, cap + 1)), bool(seed & 1), bool(seed & 2), bool(seed & 4)
    heuristic = None if seed % 3 == 0 else S.WalkHeuristic(np.where(rs.rand(K) < 0.3, 0, rs.randint(1, 9, K)).astype(np.int32), ('min', 'max')[seed & 1])
    lut = np.zeros(64, np.int32)
    lut[:22] = rs.randint(0, 50, 22)
    model, held = KV.KeyValueModel(), {}
    g, bucket, open_f, h_list = [VALUE_NONE] * pool, [-1] * pool, {}, [0] * pool
    slot_of = [-1] * n_buckets
    for s in range(6):                                                                 # slots opened earlier, one of them at the top of the range
        g[s], bucket[s] = int(rs.randint(0, 30)), s
        open_f[s], slot_of[s] = g[s] + int(rs.randint(0, 5)), s
    g[5] = open_f[5] = VALUE_NONE - 1
    f_np, h_np, g_np, bucket_np, sob_np = np.full(pool, VALUE_NONE, np.int32), np.zeros(pool, np.int32), np.array(g, np.int32), np.array(bucket, np.int32), np.array(slot_of, np.int32)
    for s, x in open_f.items():
        f_np[s] = x
    cursor, goal = 6, (VALUE_NONE, -1)
    chose_some = superseded_some = pruned_some = False
    for it in range(4):
        keys = rs.randint(0, n_buckets, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)            # duplicates, and key 0
        where = np.array([int(k // 0x9E3779B97F4A7C15) - 1 if k else -1 for k in keys.tolist()], np.int32)   # bucket = the key's number - 1
        keys[where == n_buckets - 2] = 0                                                                # (keep the buckets below n_buckets - 1)
        where[where == n_buckets - 2] = -1
        code, msg = rs.randint(0, 22, n), np.where(rs.rand(n) < 0.3, 14, rs.randint(0, 14, n))
        info = (rs.randint(0, 2, n) | ((rs.rand(n) < 0.3).astype(np.int64) << 1) | (code << 2) | (msg << 8)).astype(np.uint32)
        dist = rs.randint(-1, 12, (cap, K)).astype(np.int32)
        # the brute-force statement
        cand = sorted((x, s) for s, x in open_f.items())
        picked = sorted(s for _, s in cand[:keep])
        old = [open_f.pop(s) for s in picked]
        parents = [IDX_NONE if prune and x >= goal[0] else s for s, x in zip(picked, old)] + [IDX_NONE] * (cap - len(picked))
        e = brute_force(parents, g, bucket, info, keys, where, model, cursor, A, lut, by_action, None, stop, goal, pool)
        e_superseded = 0
        for c in e['next_parents']:
            if c == IDX_NONE:
                continue
            earlier = slot_of[bucket[c]]
            if earlier >= 0 and earlier != c:
                open_f.pop(earlier, None)
                e_superseded += 1
            slot_of[bucket[c]] = c
        for k, c in enumerate(e['next_parents']):
            if c != IDX_NONE:
                h_list[c] = 0 if heuristic is None else brute_h(dist[k], heuristic.weights, heuristic.mode)
                open_f[c] = min(g[c] + h_list[c], VALUE_NONE - 1)
        # the numpy references
        r = S.best_first_reference(f_np, h_np, g_np, bucket_np, sob_np, lambda p: (info, keys, where), held, cursor, A, lut, by_action, keep, cap, stop,
                                   S.SearchGoal(*goal), prune, heuristic, lambda c: dist, pool)
        assert isinstance(r, S.BestFirst) and r.chosen.tolist() == picked + [IDX_NONE] * (cap - len(picked)) and r.parents.tolist() == parents, it
        assert (r.pruned, r.open, r.superseded) == (sum(p == IDX_NONE for p in parents[:len(picked)]), len(cand), e_superseded), it
        assert (r.f_min, r.f_bound) == ((min(old), max(old)) if old else (VALUE_NONE, VALUE_NONE)), it
        assert r.relaxed.next_parents.tolist() == e['next_parents'] and r.relaxed.cursor == e['cursor'] and tuple(r.relaxed.goal) == e['goal'], it
        assert f_np.tolist() == [open_f.get(s, VALUE_NONE) for s in range(pool)], (it, 'f')
        assert h_np.tolist() == h_list and g_np.tolist() == g and bucket_np.tolist() == bucket and sob_np.tolist() == slot_of, it
        cursor, goal = e['cursor'], e['goal']
        chose_some, superseded_some, pruned_some = chose_some or bool(picked), superseded_some or e_superseded > 0, pruned_some or r.pruned > 0
    assert chose_some
    return superseded_some, pruned_some


@pytest.mark.parametrize('seed', range(12))
def test_the_references_against_a_brute_force_open_list(seed):
    random_open_list(seed)


def test_the_random_inputs_supersede_and_prune():
    hits = [random_open_list(seed) for seed in range(12)]
    assert any(s for s, _ in hits), "no random input superseded a slot"
    assert any(p for _, p in hits), "no random input pruned a slot"


def test_take_reference_edges():
    f = np.array([5, VALUE_NONE, 5, 3, VALUE_NONE - 1, 9], np.int32)
    chosen, parents, pruned, n_open, lo, hi = S.take_reference(f, 3, 4, goal_value=5, prune=True)
    assert chosen.tolist() == [0, 2, 3, IDX_NONE] and parents.tolist() == [IDX_NONE, IDX_NONE, 3, IDX_NONE]       # ties: the smaller slots; 5 >= 5 is pruned
    assert (pruned, n_open, lo, hi) == (2, 5, 3, 5) and f.tolist() == [VALUE_NONE, VALUE_NONE, VALUE_NONE, VALUE_NONE, VALUE_NONE - 1, 9]
    chosen, parents, pruned, n_open, lo, hi = S.take_reference(f, 4, 4)
    assert chosen.tolist() == [4, 5, IDX_NONE, IDX_NONE] and parents.tolist() == chosen.tolist() and (pruned, n_open, lo, hi) == (0, 2, 9, VALUE_NONE - 1)
    assert S.take_reference(f, 4, 4)[2:] == (0, 0, VALUE_NONE, VALUE_NONE) and (f == VALUE_NONE).all()


# ------------------------------------------------------------------ the model
def test_the_whole_open_list_is_the_layered_search():
    """keep >= everything open, h = 0, no pruning, beside key_value_oracle.label_correcting: iteration for iteration the same keys with the
    same values - every open state is a child of the last iteration, so choosing them all is the layered search."""
    spec, st = oracle_env()
    costs = KV.synthetic_costs(spec)
    A = spec.compile().n_actions
    cpu = KV.label_correcting(spec, st, costs, 4)
    m = model_of(spec, st, CAP, costs=costs)
    model, e_keys, _, _ = next(cpu)
    assert set(m.table.held) == set(model.held) and m.parents == [IDX_NONE] * CAP and m.f[:4] == [0] * 4 and m.f[4:] == [VALUE_NONE] * (CAP_POOL - 4)
    for it in range(4):
        rec = m.iterate()
        model, e_keys, e_values, e_best = next(cpu)
        P = len(e_keys) // A
        assert rec['chosen'] == rec['open'] == P and rec['pruned'] == 0, it
        assert (rec['keys'][:P * A] == e_keys).all() and (rec['values'][:P * A] == e_values).all() and (rec['best'][:P * A] == e_best).all(), it
        assert {k: v[0] for k, v in m.table.held.items()} == {k: v[0] for k, v in model.held.items()}, it
        assert sorted(x for x in m.f if x != VALUE_NONE) == sorted(e_values[e_best].tolist()), it      # the open list: this iteration's improved states
    assert m.table.reopened == model.reopened >= 4 and not m.full


def superseding_costs(spec):
    """KV.synthetic_costs with Right = 1 and Left = 10: three Rights (3) reach the state one Left (10) reached, while that copy is still open."""
    cs = spec.compile()
    kinds = [int(cs.act_kind[a]) for a in range(cs.n_actions)]
    costs = KV.synthetic_costs(spec).copy()
    costs[kinds.index(ACT_RIGHT)], costs[kinds.index(ACT_LEFT)] = 1, 10
    return costs


def test_a_scenario_that_supersedes():
    spec, st = oracle_env()
    m = model_of(spec, st, 1, n_roots=1, costs=superseding_costs(spec))
    first, dropped = {}, False
    for it in range(8):
        m.iterate()
        for k, v in m.table.held.items():
            dropped = dropped or v[0] < first.setdefault(k, v[0])
    superseded = sum(r['superseded'] for r in m.open_rows)
    assert superseded > 0 and dropped, "the scenario no longer supersedes"
    assert all(r['chosen'] == 1 for r in m.open_rows) and len(m.expanded_slots) == 8
    # a superseded slot is closed for good: no slot is expanded whose state a cheaper copy holds
    for slot in m.expanded_slots[1:]:
        assert m.g[slot] != VALUE_NONE
    assert len(set(m.expanded_slots)) == 8


def goal_model(heuristic, stop=False, real=True):
    """The goal state of tests/test_search_run.py from two roots, prune=True, iterated until proven() or 40 iterations.  real: the step
    costs at scale 1, keep=32, the weight 24 (the cheapest movement cost: a turn, round(24.0)) on the crafting table; else
    KV.synthetic_costs, keep=4, the weight 1 (a Left)."""
    spec, st = oracle_env(goal_state)
    w = np.zeros(len(spec.items_id), np.int32)
    w[spec.items_id['crafting_table']] = 24 if real else 1
    kw = dict(scale=1) if real else dict(costs=KV.synthetic_costs(spec))
    m = model_of(spec, st, 32 if real else 4, n_roots=2, prune=True, stop_at_goals=stop, heuristic=(w, 'min') if heuristic else None, **kw)
    while not m.proven() and len(m.iterations) < 40:
        m.iterate()
    return m


@pytest.mark.parametrize('stop', [False, True])
def test_the_goal_with_and_without_the_walk_heuristic(stop):
    """Real step costs: both searches reach the same goal value and report proven() within 40 iterations; with the walk heuristic no more
    states are expanded.  (When this was written: 499 states against 487, stop_at_goals 510 against 510.  The craft costs 8400 against 24
    to 28 a move, so every state within some 300 moves would have to be expanded before f_min reaches the goal's 8452: what ends both
    searches here is the pool of 512, exhausted - the model's `full`, F_FRONTIER_FULL on the device -, which is the proviso proven()
    documents and no proof.  The synthetic costs below give one.)"""
    assert min(int(round(STEP_COSTS[c])) for c in (1, 2)) == 24
    plain, guided = goal_model(False, stop), goal_model(True, stop)
    assert plain.proven() and guided.proven()
    assert plain.goal()[0] == guided.goal()[0] == 8452
    expanded = [sum(r['chosen'] - r['pruned'] for r in m.open_rows) for m in (plain, guided)]
    print('real costs: states expanded until proven(): h = 0 %d in %d iterations, walk heuristic %d in %d' % (expanded[0], len(plain.iterations), expanded[1], len(guided.iterations)))
    assert expanded[1] <= expanded[0]


@pytest.mark.parametrize('stop', [False, True])
def test_a_proof_with_and_without_the_walk_heuristic(stop):
    """KV.synthetic_costs (Left 1, Right 10, else 5), keep=4: both searches PROVE the goal - no state lost - at the same value, and the
    walk heuristic expands fewer states (116 against 76 when this was written)."""
    plain, guided = goal_model(False, stop, real=False), goal_model(True, stop, real=False)
    assert plain.proven() and guided.proven() and not plain.full and not guided.full
    assert plain.goal()[0] == guided.goal()[0] == 12
    assert plain.open_rows[-1]['f_min'] >= 12 and guided.open_rows[-1]['f_min'] >= 12 and plain.open_rows[-1]['open'] > 0
    expanded = [sum(r['chosen'] - r['pruned'] for r in m.open_rows) for m in (plain, guided)]
    print('synthetic costs: states expanded until proven(): h = 0 %d in %d iterations, walk heuristic %d in %d' % (expanded[0], len(plain.iterations), expanded[1], len(guided.iterations)))
    assert expanded == [116, 76]                                                       # (the figures DESIGN.md 4.26 and the README quote)
    # the heuristic is admissible on the way: h of an expanded slot is at most what the goal still costs from there
    assert all(guided.g[s] + guided.h[s] <= 12 for s in guided.expanded_slots)


def test_a_pool_beyond_the_selection_limit_is_refused_on_the_host():
    """Search.__init__ on stand-ins for the snapshot and the table: a pool of 2^24 + 1 slots is refused before the library is called, one of
    exactly 2^24 is not (it gets as far as the library call, which the stand-in's NULL handle fails)."""
    env = types.SimpleNamespace(n_actions=5, n_items=3, _h=None, device=0)
    table = types.SimpleNamespace(_open_for=lambda e: None, _valued=lambda: None, _t=None)
    for capacity, refused in (((1 << 24) + 1, True), (1 << 24, False)):
        snap = types.SimpleNamespace(env=env, capacity=capacity, _open=lambda: None, _s=None)
        with pytest.raises(ValueError if refused else Exception, match='2\\^24' if refused else None) as e:
            S.Search(snap, table, 16, keep=4, open_list=True)
        assert refused or '2^24' not in str(e.value)
        with pytest.raises(Exception) as e:                                            # a closed search has no such limit
            S.Search(snap, table, 16, keep=4)
        assert '2^24' not in str(e.value)


# ------------------------------------------------------------------ header and binding
def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    for name, value in (('NONE', _cabi.SEARCH_H_NONE), ('MIN', _cabi.SEARCH_H_MIN), ('MAX', _cabi.SEARCH_H_MAX)):
        assert int(re.search(r'#define NGW_SEARCH_H_%s (\d+)' % name, text).group(1)) == value
    assert re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    L = _cabi.lib()
    for name in ('ngw_search_create_open', 'ngw_search_read_open'):
        assert name in _cabi.SYMBOLS and getattr(L, name).argtypes, name
    assert C.sizeof(_cabi.SearchOpenReport) == 16 + 24 * _cabi.SEARCH_ROWS and C.sizeof(_cabi.SearchArraysOpen) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_cabi.SearchOptions) == 48 and _cabi.SearchOptions.weights_host.offset == 40
    assert C.sizeof(_cabi.SearchReport) == 40 + 16 * _cabi.SEARCH_ROWS                  # ngw_search_report keeps its layout
    assert L.ngw_search_create_open(None, None, None, None, None, None) == _cabi.E_INVALID_ARG and L.ngw_search_read_open(None, None, None) == _cabi.E_INVALID_ARG
