"""Valued key tables without a GPU (key_table.py insert_min / read / get / trace; include/ngw.h ngw_key_table_create_valued / _insert_min /
_read / _trace): the plain-Python statements of both contracts (key_table.insert_min_reference, trace_reference) against the dict model
of tests/key_value_oracle.py on random batches, the host-side argument checks - which raise before anything would launch -, the step-cost
values, the header / binding agreement, and the label-correcting search of tests/test_key_values.py run on the CPU oracle alone: for
the seed committed there, a stored state IS reopened."""
import os
import re

import numpy as np
import pytest

import expand_oracle as XO
import key_table_oracle as KT
import key_value_oracle as KV
import ngw_testlib as T
import snapshot_oracle as SO
from gym_novel_gridworlds_amd import _cabi, key_table as K
from gym_novel_gridworlds_amd.spec import IDX_NONE, STEP_COSTS, make_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def test_constants_agree_with_the_header_and_the_oracle():
    text = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    assert re.search(r'#define NGW_VALUE_NONE INT32_MAX\b', text) and re.search(r'#define NGW_TAG_ROOT \(-1\)', text)
    assert int(re.search(r'#define NGW_TRACE_MAX_STEPS (\d+)', text).group(1)) == K.TRACE_MAX_STEPS
    assert K.VALUE_NONE == KV.NONE == I32_MAX and K.TAG_ROOT == KV.ROOT == -1 and KV.IDX_NONE == IDX_NONE


def test_the_binding_names_the_new_entry_points():
    """As tests/test_cabi_symbols.py states it: every symbol the header declares is in _cabi.SYMBOLS and in the library, and nothing else."""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(ngw_[a-z_0-9]+)\s*\(', text)))
    new = ['ngw_key_table_create_valued', 'ngw_key_table_insert_min', 'ngw_key_table_read', 'ngw_key_table_trace']
    assert set(new) <= set(declared) and sorted(_cabi.SYMBOLS) == declared
    L = _cabi.lib()
    for name in new:
        assert hasattr(L, name) and getattr(L, name).argtypes, name
    assert L.ngw_abi_version() == 3


def random_batch(rs, n, n_keys, special=True):
    keys = rs.randint(0, n_keys + 1, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)      # (0 stays 0: never stored)
    values = rs.randint(-5, 6, n).astype(np.int64)
    if special:
        pick = rs.rand(n)
        values = np.where(pick < 0.1, I32_MAX, np.where(pick < 0.15, I32_MIN, np.where(pick < 0.2, I32_MAX - 1, values)))
    return keys, values.astype(np.int32), rs.randint(I32_MIN, I32_MAX, n).astype(np.int32)


@pytest.mark.parametrize('seed', range(6))
def test_insert_min_reference_against_the_model(seed):
    """Eight calls of up to 300 positions over 40 keys: many copies of a key in one call, equal values inside a call and across calls,
    VALUE_NONE as a value, key 0, calls without tags, refused positions."""
    rs = np.random.RandomState(seed)
    model, held = KV.KeyValueModel(), {}
    for call in range(8):
        n = int(rs.randint(0, 300))
        keys, values, tags = random_batch(rs, n, 40)
        tags = None if call % 3 == 2 else tags
        refused = rs.rand(n) < 0.05 if call % 4 == 3 else None
        e_fresh, e_stored, e_best = model.insert_min(keys, values, tags, refused)
        stored, fresh, best = K.insert_min_reference(held, keys, values, tags, refused)
        assert (stored == e_stored).all() and (fresh == e_fresh).all() and (best == e_best).all(), call
        assert {k: tuple(v) for k, v in held.items()} == {k: tuple(v) for k, v in model.held.items()}, call
        for k in set(keys[e_stored].tolist()):
            assert int(best[(keys == k) & e_stored].sum()) <= 1
    assert model.reopened > 0 and len(model) > 30


def test_insert_min_reference_states_the_contract_in_small():
    held = {}
    stored, fresh, best = K.insert_min_reference(held, [7, 7, 0, 7, 9], [5, 3, 1, 3, K.VALUE_NONE], [10, 11, 12, 13, 14])
    assert stored.tolist() == [True, True, False, True, True] and fresh.tolist() == [True, False, False, False, True]
    assert best.tolist() == [False, True, False, False, False]                   # the smallest (value, position); VALUE_NONE offers nothing
    assert held == {7: [3, 11], 9: [K.VALUE_NONE, K.TAG_ROOT]}
    _, fresh, best = K.insert_min_reference(held, [7, 9, 7], [3, I32_MIN, 4])    # an equal value is no improvement; no tags: the tag stays
    assert not fresh.any() and best.tolist() == [False, True, False] and held == {7: [3, 11], 9: [I32_MIN, K.TAG_ROOT]}


@pytest.mark.parametrize('seed', range(4))
def test_trace_reference_against_the_model(seed):
    """Random tags over 32 buckets, a third of them empty: roots, chains, cycles, tags out of range and tags into empty buckets."""
    rs = np.random.RandomState(100 + seed)
    buckets, A = 32, 5
    occupied = rs.rand(buckets) < 0.7
    tags = np.where(rs.rand(buckets) < 0.25, -1, rs.randint(-3, buckets * A + 4, buckets)).astype(np.int32)
    where = np.r_[np.arange(-2, buckets + 2), IDX_NONE].astype(np.int32)
    of_bucket = {b: int(tags[b]) for b in range(buckets) if occupied[b]}
    seen_bad = set()
    for steps in (0, 1, 3, 8):
        for lo in list(range(len(where))) + [None]:               # (the flag is one per call: one query a call, then all of them in one)
            w = where if lo is None else where[lo:lo + 1]
            exp = KV.trace(w, steps, A, of_bucket, buckets)
            got = K.trace_reference(w, steps, A, occupied, tags)
            for g, e in zip(got[:3], exp[:3]):
                assert g.dtype == np.int32 and g.shape == e.shape and (g == e).all(), (steps, lo)
            assert got[3] == exp[3], (steps, lo)
            seen_bad.add(got[3])
    assert seen_bad == {False, True}


def test_trace_reference_states_the_contract_in_small():
    occupied = np.array([1, 1, 1, 1, 0, 1, 1, 0], bool)
    #                 0: root   1 <- 0 by action 2   2 <- 1 by action 0   3 <- 2 by action 1   5 <-> 6: a cycle
    tags = np.array([-1, 0 * 3 + 2, 1 * 3 + 0, 2 * 3 + 1, -1, 6 * 3 + 0, 5 * 3 + 1, -1], np.int32)
    plans, length, root, bad = K.trace_reference([0, 1, 3, 5, -1, IDX_NONE], 3, 3, occupied, tags)
    assert length.tolist() == [0, 1, 3, -1, -1, -1] and root.tolist() == [0, 0, 0, -1, -1, -1] and not bad
    assert plans.T.tolist() == [[-1, -1, -1], [2, -1, -1], [2, 0, 1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    plans, length, root, bad = K.trace_reference([3], 2, 3, occupied, tags)          # T + 1 links: too long, and no flag
    assert length.tolist() == [-1] and root.tolist() == [-1] and (plans == -1).all() and not bad
    for w, tg in ((4, None), (8, None), (1, 7 * 3), (1, 8 * 3), (1, -2)):             # an empty bucket, one out of range; tags into / beyond / below
        t2 = tags.copy()
        if tg is not None:
            t2[1] = tg
        plans, length, root, bad = K.trace_reference([w], 3, 3, occupied, t2)
        assert length.tolist() == [-1] and root.tolist() == [-1] and (plans == -1).all() and bad, (w, tg)


def valued_stand_in(capacity=8):
    t = KT.stand_in_table(capacity)
    t.values = True
    return t


def test_host_side_checks_raise_before_anything_launches():
    """Through key_table_oracle.stand_in_table: no library call, no device - every one of these raises in the argument checks."""
    t = valued_stand_in()
    keys = np.arange(1, 5, dtype=np.uint64)
    for values, match in ((np.zeros(4, np.float32), 'values: integers'), (np.zeros((2, 2), np.int32), 'values: a one-dimensional'),
                          (np.zeros(3, np.int32), 'values: 3 entries for 4 keys'), ([0, 1, 2, 1 << 31], 'values: an entry does not fit'),
                          (None, 'values')):
        with pytest.raises(ValueError, match=match):
            t.insert_min(keys, values)
    for tags, match in ((np.zeros(4, np.float64), 'tags: integers'), (np.zeros((4, 1), np.int32), 'tags: a one-dimensional'),
                        (np.zeros(5, np.int32), 'tags: 5 entries for 4 keys'), ([0, 0, 0, -(1 << 31) - 1], 'tags: an entry does not fit')):
        with pytest.raises(ValueError, match=match):
            t.insert_min(keys, np.zeros(4, np.int32), tags)
    with pytest.raises(ValueError, match='keys: integer keys'):
        t.insert_min(np.zeros(4, np.float32), np.zeros(4, np.int32))
    import torch
    with pytest.raises(ValueError, match='values: a contiguous one-dimensional int32 tensor'):
        t.insert_min(keys, torch.zeros(4, dtype=torch.int64))                       # a tensor of the wrong dtype (and device)
    with pytest.raises(ValueError, match='where: integers'):
        t.read(np.zeros(3, np.float32))
    with pytest.raises(ValueError, match='where: a one-dimensional'):
        t.read(np.zeros((3, 1), np.int32))
    with pytest.raises(ValueError, match='steps'):
        t.trace([0], -1)
    with pytest.raises(ValueError, match='steps'):
        t.trace([0], K.TRACE_MAX_STEPS + 1)
    with pytest.raises(ValueError, match='n_actions'):
        t.trace([0], 4, n_actions=0)
    with pytest.raises(ValueError, match='where: integers'):
        t.trace(np.zeros(2, np.float32), 4)


def test_calls_on_a_table_without_values_are_refused():
    t = KT.stand_in_table()
    for call in (lambda: t.insert_min([1], [1]), lambda: t.read([0]), lambda: t.get([1]), lambda: t.trace([0], 4)):
        with pytest.raises(ValueError, match='without values'):
            call()


def test_trace_refuses_tags_that_would_not_fit():
    """buckets * A beyond 2^31 - 1: capacity 2^28 is 2^29 buckets, times the 5 actions of the stand-in env ... and times 4 exactly 2^31."""
    t = valued_stand_in(1 << 28)
    assert t.buckets == 1 << 29
    for A in (None, 4):
        with pytest.raises(ValueError, match='does not fit a tag'):
            t.trace([0], 4, n_actions=A)
    small = valued_stand_in(8)
    with pytest.raises(ValueError, match='does not fit a tag'):
        small.trace([0], 4, n_actions=1 << 27)                                     # 16 buckets * 2^27 = 2^31


@pytest.mark.parametrize('scale', [1, 3, 0.5, 100])
def test_step_cost_values(scale):
    codes = np.arange(len(STEP_COSTS))
    rs = np.random.RandomState(5)
    words = (rs.randint(0, 4, len(codes)) | (codes << 2) | (rs.randint(0, 16, len(codes)) << 8) | (rs.randint(0, 1 << 12, len(codes)) << 16)).astype(np.uint32)
    exp = np.array([round(STEP_COSTS[c] * scale) for c in codes], np.int32)
    got = K.step_cost_values(words, scale)
    assert got.dtype == np.int32 and (got == exp).all()
    assert (K.step_cost_values(words.reshape(2, -1), scale) == exp.reshape(2, -1)).all()
    import torch
    tw = torch.from_numpy(words.view(np.int32).copy())                               # the words as torch carries them: int32 over the same bits
    tg = K.step_cost_values(tw, scale)
    assert tg.dtype == torch.int32 and (tg.numpy() == exp).all()
    assert min(STEP_COSTS[1:]) == 24.0 and max(STEP_COSTS) == 50000


def test_step_cost_values_refuses_a_scale_that_reaches_value_none():
    with pytest.raises(ValueError, match='scale'):
        K.step_cost_values(np.zeros(1, np.uint32), 1 << 16)                          # 50 000 * 65 536 > 2^31
    with pytest.raises(ValueError, match='scale'):
        K.step_cost_values(np.zeros(1, np.uint32), -1)


def test_the_search_of_the_gpu_test_reopens_a_state_on_the_cpu_oracle():
    """tests/test_key_values.py's label-correcting search, the model alone: with the committed seed and the synthetic costs a state stored
    in iteration 1 (by one Right, 10) is improved in iteration 3 (by three Lefts, 3) - per env -, and every improved position's value is
    what the model holds for its key afterwards."""
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, 9)
    n = 4
    o = Oracle(spec.compile(), n, seed=XO.good_seed(spec, n))
    o.reset()
    costs = KV.synthetic_costs(spec)
    assert sorted(set(costs.tolist())) == [1, 5, 10] and int((costs == 1).sum()) == 1 and int((costs == 10).sum()) == 1
    reopened, sizes = [], []
    for model, keys, values, best in KV.label_correcting(spec, SO.oracle_state(o), costs, 4):
        reopened.append(model.reopened)
        sizes.append((len(keys), int(best.sum())))
        held = model.get(keys[best])[0]
        assert (held == values[best]).all()
    assert reopened[:3] == [0, 0, 0] and reopened[3] >= n and reopened[4] > reopened[3], reopened
    assert max(s[1] for s in sizes) < 256 and sum(s[1] for s in sizes) < 512          # (what the GPU test sizes its frontier and pool by)
