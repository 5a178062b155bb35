"""The wide specs of tests/wide_specs.py on the MI355X: K = 20, 21 and 24 items, A = 31 to 48 actions, 8 recipes - the limits of the ABI, which
no other test comes near (their largest spec has 13 items and 20 actions).  Every expectation is the CPU oracle's or a CPU model's, bit for
bit; tests/test_wide_specs_cpu.py asserts on the same seeds that the wide columns are in play.  Shapes: 65 envs (a wave and one), 130 pairs,
T = 6 to 8, key tables of 4096, tree tables of 64 buckets for the stages alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import expand_oracle as XO
import frontier_oracle as FO
import key_table_oracle as KT
import lookahead_oracle as LO
import mask_oracle as M
import playout_oracle as PO
import sample_oracle as SA
import slot_observe_oracle as OO
import snapshot_oracle as SO
import state_key_oracle as SK
import successor_key_oracle as SKO
import test_step_plain as SP
import test_search_specs_cpu as XS
import test_trajectories as TT
import test_trajectory_views as TV
import test_tree_rule_cpu as XR
import test_wide_specs_cpu as X
import trajectory_oracle as TO
import trajectory_view_oracle as VO
import tree_oracle as TM
import walk_oracle as WO
import wide_specs as W
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd import search as S
from gym_novel_gridworlds_amd.frontier import select_reference
from gym_novel_gridworlds_amd.key_table import TAG_ROOT, VALUE_NONE, insert_min_reference, step_cost_values, trace_reference
from gym_novel_gridworlds_amd.lidar import LidarConfig
from gym_novel_gridworlds_amd.search import RecipeHeuristic
from gym_novel_gridworlds_amd.state_keys import KEY_STATE
from gym_novel_gridworlds_amd.tree import backup_reference, spread_rows_reference
from gym_novel_gridworlds_amd.walk import walk_action_ids

pytestmark = pytest.mark.gpu
N, PAIRS, T_, SEED = W.N_ENVS, W.N_PAIRS, 6, 0x7A11CAFE5EED0004
F_BAD_WEIGHT, BUCKETS = 16, 64
STATE = SO.STATE_KEYS


@pytest.fixture(scope='module')
def envs():
    """name -> (spec, the env of 65 in the oracle's states after the warm-up, those states), made at first use and put back at every use."""
    made = {}

    def get(name):
        spec, seed = W.oracle_env(name)[:2]
        rows = W.rows_of(name)
        if name not in made:
            made[name] = VecNovelGridworld(spec=spec, num_envs=N, seed=seed)
            made[name].reset()
        v = made[name]
        v.set_state(0, **{k: rows[k] for k in STATE})
        v.error_flags()
        return spec, v, rows
    yield get
    for v in made.values():
        v.close()


_successors = {}


def successors(name):
    """Every child of every one of the 65 states, from the oracle, computed once."""
    if name not in _successors:
        _successors[name] = SKO.Successors(W.spec_of(name), W.rows_of(name), np.arange(N))
    return _successors[name]


# ------------------------------------------------------------------ a. stepping
@pytest.mark.parametrize('name, n', [(name, N) for name in W.ALL] + [('w20a33', PAIRS), ('w24a48', PAIRS)])
def test_reset_and_batched_steps(name, n):
    """The reset (full start tables), then 60 steps - the warm-up of the CPU file and 36 more, half uniform actions, half valid ones -, step by
    step: state, reward, done, info word, flags.  65 envs, and 130 on two specs.  The step kernel's instantiation is the table's."""
    from oracle.ngw_oracle import Oracle
    spec, seed, start, acts, _, _ = W.oracle_env(name, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    o = Oracle(spec.compile(), n, seed=seed)
    v.reset(); o.reset()
    XO.assert_rows(v.get_state(), SO.oracle_state(o), name + ': the reset')
    assert v.n_actions == W.TABLE[name][1] and v.n_items == W.TABLE[name][0]
    v.set_state(0, **{k: start[k] for k in STATE})
    SO.put_state(o, start)
    rs = np.random.RandomState(n)
    for t in range(60):
        a = acts[t] if t < len(acts) else W.mixed_actions(spec, o.st, rs)[0]
        dev = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        v.step_device(dev.data_ptr())
        SP._compare(v, o, o.step(a), '%s step %d' % (name, t))
        assert v.step_kernel_plain[1] is (W.TABLE[name][6] == 'plain' and SP._PLAIN_ON), name
    v.close()


@pytest.mark.parametrize('name', W.ALL)
def test_autoreset(name):
    """Autoreset with horizon 5: 36 steps, every env reset several times from the full start tables (a tight map may exhaust a placement: the
    flag is then the oracle's too)."""
    from oracle.ngw_oracle import Oracle
    spec, seed = W.oracle_env(name)[:2]
    v = VecNovelGridworld(spec=spec, num_envs=N, seed=seed, autoreset=True, horizon=5)
    o = Oracle(spec.compile(), N, seed=seed, autoreset=True, horizon=5)
    v.reset(); o.reset()
    rs = np.random.RandomState(len(name))
    for t in range(36):
        a, _ = W.mixed_actions(spec, o.st, rs)
        dev = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        v.step_device(dev.data_ptr())
        SP._compare(v, o, o.step(a), '%s autoreset step %d' % (name, t))
    assert o.st.episode.min() >= 6
    v.close()


@pytest.mark.parametrize('name', W.ALL)
def test_one_env_entry_points(name):
    """reset1 / step1 / last_state1 on a handle of one env: 40 steps, valid actions on the odd ones, every fourth one >= 32 where one is."""
    from oracle.ngw_oracle import Oracle
    spec, seed = W.oracle_env(name)[:2]
    v = VecNovelGridworld(spec=spec, num_envs=1, seed=seed)
    o = Oracle(spec.compile(), 1, seed=seed)
    v.reset1(); o.reset()
    rs, A, wide = np.random.RandomState(7), v.n_actions, 0
    inv = np.asarray(o.st.inv).copy()
    inv[0] = rs.randint(1, 4, inv.shape[1]) * np.array([int(spec.compile().breakable[k]) for k in range(inv.shape[1])])
    v.set_state(0, inv=inv.astype(np.int32))
    o.st.inv[...] = inv
    for t in range(40):
        words = M.oracle_mask_words(spec, o.st)
        valid = [b for b in range(A) if (int(words[0]) >> b) & 1]
        high = [b for b in valid if b >= 32]
        a = (high[rs.randint(len(high))] if t % 4 == 3 and high else valid[rs.randint(len(valid))]) if t & 1 and valid else int(rs.randint(A))
        got = v.step1(a)
        o.step(np.array([a], np.int32))
        assert got == (int(o.reward[0]), bool(o.done[0]), bool(o.result[0]), int(o.cost_code[0]), int(o.msg_code[0]), int(o.msg_arg[0])), (name, t, a)
        m, r, c, f, i, sel, sc = v.last_state1()
        assert m == np.ascontiguousarray(o.st.map[0], np.int8).tobytes() and i == np.ascontiguousarray(o.st.inv[0], np.int32).tobytes(), (name, t)
        assert (r, c, f, sel, sc) == (int(o.st.loc[0][0]), int(o.st.loc[0][1]), int(o.st.facing[0]), int(o.st.selected[0]), int(o.st.step_count[0])), (name, t)
        wide += a >= 32 and bool(o.result[0])
    assert wide >= 1 or A <= 32
    v.close()


# ------------------------------------------------------------------ b. masks and lookahead
@pytest.mark.parametrize('name', W.ALL)
def test_masks_and_lookahead(envs, name):
    spec, v, rows = envs(name)
    A = v.n_actions
    st = XO.rows_state(spec, rows, np.arange(N))
    words = M.oracle_mask_words(spec, st)
    assert (v.action_mask_words(copy=True) == words).all(), name
    masks = v.action_masks()
    assert masks.shape == (N, A) and (masks == M.oracle_masks(spec, st)).all()
    assert (v.action_mask_words(device=True).cpu().numpy().view(np.uint64) == words).all()
    look = v.lookahead(copy=True)
    exp = LO.oracle_lookahead(spec, st)
    assert look.reward.shape == (N, A)
    LO.assert_table(look._asdict(), exp, name + ' live envs')
    dev = v.lookahead(device=True)
    LO.assert_table(dict(reward=dev.reward.cpu().numpy(), done=dev.done.cpu().numpy(), result=dev.result.cpu().numpy(),
                         info=dev.info.cpu().numpy().view(np.uint32)), exp, name + ' device table')
    if A > 32:
        assert (words >> np.uint64(32)).any() and exp['result'][:, 32:].any()
    pool = v.snapshot(N + 4)
    pool.save(slots=np.arange(N)[::-1].copy())
    slots = np.array([N - 1, 0, 5, 5, 64, 33, 1], np.int32)
    OO.assert_masks(pool.action_masks(slots), spec, rows, N - 1 - slots, name + ' saved slots')
    v.set_action_masks(True)
    a = np.where(masks.any(1), masks.argmax(1), 0).astype(np.int32)
    v.step(a)
    v.set_action_masks(False)
    o_rows, _ = XO.oracle_expand(spec, rows, np.arange(N), a)
    assert (v.action_mask_words(copy=True) == M.oracle_mask_words(spec, XO.rows_state(spec, o_rows, np.arange(N)))).all(), name + ': the masks a step leaves'
    pool.close()


# ------------------------------------------------------------------ c. snapshots, expand, rollouts, playouts
@pytest.mark.parametrize('name', W.ALL)
def test_snapshots_and_expand(envs, name):
    spec, v, rows = envs(name)
    A = v.n_actions
    pool = v.snapshot(N + N * A)
    pool.save()
    XO.assert_rows(pool.state(0, N), rows, name + ' save')
    e = pool.expand_all(np.arange(N), N)
    succ = successors(name)
    XO.assert_rows(pool.state(N, N * A), succ.kids, name + ' expand_all')
    XO.assert_reports({k: np.asarray(getattr(e, k)).reshape(-1) for k in ('reward', 'done', 'result', 'info')},
                      {k: x.reshape(-1) for k, x in succ.rep.items()}, name + ' expand_all')
    perm = np.random.RandomState(3).permutation(N).astype(np.int32)
    pool.restore(slots=N + perm * A + (perm % A), envs=np.arange(N, dtype=np.int32))
    XO.assert_rows(v.get_state(), succ.child_rows(perm, perm % A), name + ' restore')
    now, src = succ.child_rows(perm, perm % A), np.random.RandomState(4).randint(0, N, N).astype(np.int32)
    v.fork(src)
    XO.assert_rows(v.get_state(), {k: x[src] for k, x in now.items()}, name + ' fork')
    pool.close()


_traj = {}


def traj_expected(name, steps):
    """130 pairs over the 65 states: the uniform playout, a weighted one and a rollout of random plans on the oracle, once."""
    if (name, steps) not in _traj:
        spec = W.spec_of(name)
        rows, A = W.rows_of(name), len(spec.actions_id)
        st = XO.rows_state(spec, rows, np.arange(N))
        lc = LidarConfig(spec, 8)
        rs = np.random.RandomState(steps)
        parents, plans = rs.randint(0, N, PAIRS), rs.randint(0, A, (PAIRS, steps))
        x = SA.random_weights(rs, 1, A)[0]
        x[:32] = 0 if A > 32 else x[:32]                                             # weight mass on the actions >= 32 alone
        _, _, au, _ = PO.oracle_playout(spec, st, parents, steps, SEED)
        _, _, aw, _ = SA.oracle_weighted_playout(spec, st, parents, steps, SEED, x)
        out = {}
        for kind, acts in (('playout', au), ('weighted', aw), ('rollout', plans.T)):
            out[kind] = TO.oracle_traj(spec, st, parents, acts, None, lc=lc)
            out[kind]['actions'] = acts
        _traj[(name, steps)] = (parents, plans, x, lc, out)
    return _traj[(name, steps)]


@pytest.mark.parametrize('name', W.ALL)
def test_playouts_and_rollouts_recorded(envs, name):
    """Valid-action playouts - uniform and weighted, the weights on the actions >= 32 alone where there are any -, and slot rollouts, 130 pairs,
    T = 6: reports, actions, rewards, mask words, lidar rows and path keys against the oracle."""
    spec, v, rows = envs(name)
    parents, plans, x, lc, exp = traj_expected(name, T_)
    v.lidar_configure(lc, dtype=np.int32)
    pool = v.snapshot(N)
    pool.save()
    for kind in ('playout', 'weighted'):
        p = pool.playout(parents, T_, SEED, record=True, rewards=True, masks=True, observe='lidar', path_keys=True, weights=x if kind == 'weighted' else None)
        TT.assert_result(p, exp[kind], '%s %s' % (name, kind))
    r = pool.rollout(parents, plans, rewards=True, observe='lidar', path_keys=True)
    TT.assert_result(r, exp['rollout'], name + ' rollout')
    if v.n_actions > 32:
        assert (exp['playout']['actions'] >= 32).any() and (exp['playout']['masks'] >> np.uint64(32)).any()
        assert (exp['weighted']['actions'] >= 32).mean() > 0.25, "the weights on the wide actions draw them"
    assert v.error_flags() == 0
    pool.close()


@pytest.mark.parametrize('name', [n for n in W.ALL if W.TABLE[n][0] >= 20])
def test_playouts_and_rollouts_with_agent_views(envs, name):
    """The same 130 pairs with observe='agent_view': the window, the facing id and the inventory of K = 20 to 24 columns behind every step."""
    spec, v, rows = envs(name)
    parents, plans, x, lc, exp = traj_expected(name, T_)
    st = XO.rows_state(spec, rows, np.arange(N))
    pool = v.snapshot(N)
    pool.save()
    views = {kind: VO.expect_views(spec, st, parents, exp[kind], 5) for kind in exp}
    p = pool.playout(parents, T_, SEED, record=True, rewards=True, masks=True, path_keys=True, observe='agent_view', view_size=5)
    TV.assert_result(p, exp['playout'], views['playout'], name + ' playout')
    w = pool.playout(parents, T_, SEED, record=True, weights=x, observe='agent_view', view_size=5)
    TV.assert_result(w, exp['weighted'], views['weighted'], name + ' weighted')
    r = pool.rollout(parents, plans, rewards=True, observe='agent_view', view_size=5)
    TV.assert_result(r, exp['rollout'], views['rollout'], name + ' rollout')
    inv = views['playout']['inventory_items_quantity']
    assert inv[1:, :, 12:].any() and inv[1:, :, -1].any() and VO.windows_move(views['playout'], exp['playout']['reports']['length']) > 0
    assert v.error_flags() == 0
    pool.close()


@pytest.mark.parametrize('name', W.WIDE_A)
def test_sampled_actions(envs, name):
    """Policy weights [130, A] under the mask: random rows, rows with mass on the actions >= 32 alone, rows of zeros (the uniform fallback over
    more than 32 valid actions on the A = 48 spec)."""
    spec, v, rows = envs(name)
    A = v.n_actions
    rs = np.random.RandomState(A)
    slots = rs.randint(0, N, PAIRS).astype(np.int32)
    x = SA.random_weights(rs, PAIRS, A)
    x[::3, :32] = 0
    x[1::7] = 0
    pool = v.snapshot(N)
    pool.save()
    for t in (0, 5):
        exp = SA.oracle_sample(spec, rows, slots, x, SEED, first_pair=1000, t=t)
        SA.assert_sampled(pool.sample_actions(slots, x, SEED, first_pair=1000, t=t), exp, '%s t %d' % (name, t))
        assert (exp[0] >= 32).sum() >= 8 and v.error_flags() == exp[3]
    pool.close()


# ------------------------------------------------------------------ d. keys
@pytest.mark.parametrize('name', W.ALL)
def test_keys(envs, name):
    spec, v, rows = envs(name)
    K = v.n_items
    idx = np.arange(N)
    SK.assert_keys(v.state_keys(), rows, idx, KEY_STATE, name + ' live envs')
    pool = v.snapshot(N + 8)
    pool.save()
    for fields in (KEY_STATE, SK.INV, SK.ALL, SK.MAP | SK.SELECTED):
        SK.assert_keys(pool.keys(idx.astype(np.int32), fields), rows, idx, fields, name + ' slots')
    SKO.assert_successors(pool.successor_keys(idx.astype(np.int32), SK.ALL), successors(name), SK.ALL, name + ' successor keys')
    SKO.assert_successors(v.successor_keys(fields=SK.INV | SK.SELECTED), successors(name), SK.INV | SK.SELECTED, name + ' successor keys of the envs')
    # pairs that differ in one wide place: inv[K - 1], inv[K - 2] against inv[K - 1], selected
    base = {k: np.repeat(np.asarray(rows[k])[:1], 6, axis=0) for k in STATE}
    inv = base['inv'].reshape(6, K).copy()
    inv[:, K - 2:] = 0
    inv[1, K - 1], inv[2, K - 2], inv[3, K - 1] = 1, 1, 2
    base['inv'] = inv
    base['selected'] = np.array([0, 0, 0, 0, K - 1, K - 2], np.int32)
    v.set_state(0, **{k: x for k, x in base.items()})
    pool.save(envs=np.arange(6, dtype=np.int32), slots=np.arange(N, N + 6, dtype=np.int32))
    got = SK.as_u64(pool.keys(np.arange(N, N + 6, dtype=np.int32), KEY_STATE))
    assert got.tolist() == SK.keys_of(base, np.arange(6), KEY_STATE).tolist() and len(set(got.tolist())) == 6, name + ': the pairs'
    assert SK.as_u64(v.state_keys(np.arange(6, dtype=np.int32))).tolist() == got.tolist()
    pool.close()


# ------------------------------------------------------------------ e. tables, recipe bound, walk distances
@pytest.mark.parametrize('name', ['w20a33', 'w21', 'w24a48'])
def test_tables_recipe_costs_and_walks(envs, name):
    spec, v, rows = envs(name)
    K, A = v.n_items, v.n_actions
    pool, table = v.snapshot(N), v.key_table(W.KEYS)
    pool.save()
    model, book = KT.KeyTableModel(), KT.WhereBook(table.buckets)
    succ = successors(name)
    keys = succ.keys(KEY_STATE).reshape(-1)                                          # 65 * A keys, many repeated
    fresh, stored = model.insert(keys)
    got = table.insert(keys)
    assert (np.asarray(got.fresh).astype(bool) == fresh).all() and len(table) == len(model) > N
    book.check(keys, got.where, stored, name + ' insert')
    _, ins = pool.insert_successor_keys(table)
    assert not np.asarray(ins.fresh).any(), "every successor key is held already"
    book.check(keys, np.asarray(ins.where).reshape(-1), stored, name + ' insert_successor_keys')
    program = S.recipe_program(spec, None, 1)
    want = S.recipe_cost_reference(rows['inv'], S.map_item_counts(rows['map'], K), program)
    assert pool.recipe_costs().tolist() == want.tolist() == v.recipe_costs().tolist() and len(set(want.tolist())) > 2
    idx = np.arange(0, N, 4)
    dist, _, _ = WO.walk_rows(rows, idx, K, None, 0, walk_action_ids(spec))
    got = pool.walk_distances(idx.astype(np.int32))
    assert got.dtype == np.int32 and got.shape == dist.shape == (len(idx), K) and (got == dist).all(), np.argwhere(got != dist)[:2]
    assert (dist[:, 12:] > 0).any(), "an item with id >= 12 is reached by a walk"
    pool.close()
    table.close()


@pytest.mark.parametrize('name', ['w20a33', 'w21', 'w24a48'])
def test_valued_tables_frontiers_and_traces(envs, name):
    """insert_keys_min of the 65 states as roots, insert_min of their 65 * A successor keys under the step costs with tags = bucket * A + action,
    a compaction and a selection over the [65, A] arrays (65 * A = 1, 2 and 0 mod 4 over the three specs), and trace with n_actions = A."""
    spec, v, rows = envs(name)
    A = v.n_actions
    pool, table = v.snapshot(N), v.key_table(W.KEYS, values=True)
    pool.save()
    succ = successors(name)
    held = {}
    root_keys = SK.keys_of(rows, np.arange(N), KEY_STATE)
    stored, fresh, best = insert_min_reference(held, root_keys, np.zeros(N, np.int32))
    got_keys, got = pool.insert_keys_min(table, np.arange(N, dtype=np.int32), np.zeros(N, np.int32))
    assert got_keys.tolist() == root_keys.tolist()
    assert ((got.where >= 0) == stored).all() and (got.fresh == fresh).all() and (got.best == best).all(), name + ': the roots'
    keys = succ.keys(KEY_STATE).reshape(-1)
    values = np.where(succ.rep['result'], step_cost_values(succ.rep['info'], 1), VALUE_NONE).astype(np.int32).reshape(-1)
    tags = (np.repeat(got.where.astype(np.int64), A) * A + np.tile(np.arange(A), N)).astype(np.int32)
    stored, fresh, best = insert_min_reference(held, keys, values, tags)
    kb = table.insert_min(keys, values, tags, device=True)
    where = kb.where.cpu().numpy()
    assert ((where >= 0) == stored).all() and (kb.fresh.cpu().numpy() == fresh).all() and (kb.best.cpu().numpy() == best).all(), name + ': the successors'
    assert best.reshape(N, A)[:, 32:].any() or A <= 32
    value, tag = table.read(where)
    assert value.tolist() == [held[k][0] for k in keys.tolist()] and tag.tolist() == [held[k][1] for k in keys.tolist()]
    # a compaction of the improving offers and a selection of the 5 cheapest per state
    parents = torch.arange(N, dtype=torch.int32, device=kb.best.device) + 1000
    flags = kb.best.view(torch.uint8).reshape(N, A).contiguous()
    total = int(best.sum())
    for capacity in (total + 5, total - 3):
        fr = pool.frontier(capacity)
        v.error_flags()
        first, second = fr.compact(flags, div=A, map=parents)
        e1, e2, count, full = FO.compact(best, A, np.arange(N) + 1000, capacity)
        assert first.cpu().numpy().tolist() == e1.tolist() and second.cpu().numpy().tolist() == e2.tolist(), (name, capacity)
        assert [fr.count(), fr.total()] == count and v.error_flags() == (FO.F_FRONTIER_FULL if full else 0) and full == (capacity < total)
        fr.close()
    fr = pool.frontier(N * 5)
    vals = torch.from_numpy(values).to(kb.best.device)
    sel = fr.select(vals, 5, div=A, map=parents, flags=flags.reshape(-1), groups=N)
    e1, e2, taken, bound, count = select_reference(values, 5, A, (np.arange(N) + 1000).astype(np.int32), best, N)
    assert sel.first.cpu().numpy().tolist() == e1.tolist() and sel.second.cpu().numpy().tolist() == e2.tolist(), name + ': select'
    assert sel.taken.cpu().numpy().tolist() == taken.tolist() and sel.bound.cpu().numpy().tolist() == bound.tolist()
    assert (e2 >= 32).any() or A <= 32
    fr.close()
    # the way back under tag = bucket * A + action
    occupied, tags_of = np.zeros(table.buckets, bool), np.full(table.buckets, TAG_ROOT, np.int64)
    ks = np.array(list(held), np.uint64)
    at = table.lookup(ks)
    occupied[at] = True
    tags_of[at] = [held[k][1] for k in ks.tolist()]
    tr = table.trace(where, 4)
    plans, length, root, bad = trace_reference(where, 4, A, occupied, tags_of)
    assert (tr.plans == plans).all() and (tr.length == length).all() and (tr.root == root).all() and not bad and v.error_flags() == 0
    assert (length == 1).any() and (length == 0).any() and ((plans[0] >= 32).any() or A <= 32)
    pool.close()
    table.close()


@pytest.mark.parametrize('name', ['w20a33', 'w24a48'])
def test_a_best_first_run_under_the_recipe_heuristic(envs, name):
    """The open list under the recipe term of the spec's own program of 8 recipes, pruning, keep 8, 8 roots among 65 saved states, lists of 1024
    entries: the roots and three iterations against RecipeBestFirstModel, then h of every reached slot against recipe_cost_reference."""
    from test_best_first import assert_open, run_both
    spec, v, rows = envs(name)
    pool, table = v.snapshot(2048), v.key_table(W.KEYS, values=True)
    pool.save(envs=np.arange(N), slots=np.arange(N))
    program = S.recipe_program(spec, None, 1)
    m = XS.recipe_model(spec, pool.state(0, N), N, walk=None, capacity=1024, cap_pool=2048, keep=8, prune=True)
    s = pool.search(table, 1024, scale=1, keep=8, open_list=True, prune=True, heuristic=RecipeHeuristic(None))
    assert s.recipe == program == m.program
    s.reset_cursor(N)
    s.start(np.arange(8))
    m.start(np.arange(8))
    assert_open(v, s, pool, table, m, name + ': the roots', flags=0)
    for it in range(3):
        taken = run_both(s, m)
        assert_open(v, s, pool, table, m, '%s, iteration %d' % (name, it), flags=0)
        assert s.chosen.cpu().numpy().tolist() == taken[0], "iteration %d: the chosen slots" % it
    reached = np.array(XS.reached(m))
    st = pool.state(0, int(reached.max()) + 1)
    want = S.recipe_cost_reference(st['inv'], S.map_item_counts(st['map'], v.n_items), program)[reached]
    assert s.h.cpu().numpy()[reached].tolist() == want.tolist() and len(set(want.tolist())) > 1 and len(reached) > 64 and not m.full
    for x in (s, pool, table):
        x.close()


def test_item_masks_past_bit_16():
    """The host's 32-bit item masks (breakable, entity, break reward) at ids 16 to 23: w24a48 with two entities and a break reward there; every
    state gets item 12 + i % 12 into the cell in front of the agent, and every action's outcome and child is the oracle's."""
    name = 'w24e'
    spec, rows = W.spec_of(name), {k: np.array(x) for k, x in W.rows_of('w24a48').items()}
    size, K = spec.map_size, len(spec.items_id)
    maps, loc = rows['map'].reshape(N, size, size), rows['loc'].reshape(N, 2)
    put = 0
    for i in range(N):
        dr, dc = ((-1, 0), (1, 0), (0, -1), (0, 1))[int(rows['facing'][i])]
        r, c = int(loc[i, 0]) + dr, int(loc[i, 1]) + dc
        if 0 < r < size - 1 and 0 < c < size - 1:
            maps[i, r, c] = 12 + i % 12
            put += 1
    assert put > 48
    v = VecNovelGridworld(spec=spec, num_envs=N, seed=W.oracle_env('w24a48')[1])
    v.reset()
    v.set_state(0, **{k: rows[k] for k in STATE})
    succ = SKO.Successors(spec, rows, np.arange(N))
    look = v.lookahead(copy=True)
    LO.assert_table(look._asdict(), {k: succ.rep[k] for k in ('reward', 'done', 'result', 'info')}, name)
    pool = v.snapshot(N + N * v.n_actions)
    pool.save()
    pool.expand_all(np.arange(N), N)
    XO.assert_rows(pool.state(N, N * v.n_actions), succ.kids, name + ' expand_all')
    cs, left, brk = spec.compile(), spec.actions_id['Left'], spec.actions_id['Break']
    grabbed = [i for i in range(N) if cs.entity[12 + i % 12] and 12 + i % 12 >= 16 and
               succ.kids['inv'][i * v.n_actions + left][12 + i % 12] == rows['inv'][i][12 + i % 12] + 1]
    assert grabbed, "no step grabs an entity with id >= 16 from the cell in front"
    assert any(succ.rep['reward'][i, brk] > 0 and 12 + i % 12 >= 16 for i in range(N)), "no Break of an item with id >= 16 is rewarded"
    assert v.error_flags() == 0
    v.close()


# ------------------------------------------------------------------ f. lidar and views
@pytest.mark.parametrize('name', ['w21', 'w24'])
def test_lidar_and_agent_views(envs, name):
    spec, v, rows = envs(name)
    lc = LidarConfig(spec, 8)
    v.lidar_configure(lc, dtype=np.int32)
    idx = np.arange(N)
    OO.assert_lidar(v, v.lidar_observation(copy=True), spec, lc, rows, idx, name + ' live envs')
    pool = v.snapshot(N)
    pool.save()
    OO.assert_lidar(v, pool.lidar_observation(idx.astype(np.int32)), spec, lc, rows, idx, name + ' slots')
    OO.assert_view(pool.agent_view(idx.astype(np.int32), 5), rows, idx, 5, name + ' agent view of the slots')
    exp = OO.expect_lidar(spec, lc, rows, idx)
    assert exp[:, -1].any() and exp[:, :8 * (v.n_items - 2)].reshape(N, 8, -1)[:, :, 11:].any(), "a wide channel and the last inventory column are seen"
    pool.close()


# ------------------------------------------------------------------ g. the tree stages alone at A = 33, 40 and 48
def tree_spec(A):
    if A == 33:
        return W.spec_of('w20a33')
    if A == 48:
        return W.spec_of('w24a48')
    import copy
    spec = copy.deepcopy(W.spec_of('w24'))                                           # A = 40: w24 and two aliases
    spec.add_alias('Select_zinc')
    spec.add_alias('Forward')
    return spec


def small_env(A):
    v = VecNovelGridworld(spec=tree_spec(A), num_envs=4, seed=9)
    v.reset()
    assert v.n_actions == A
    return v


def fill(t, A, rs, priors):
    v, r, m = XR.random_rows(rs, BUCKETS, A)
    cv, cr, cm, cp, _ = W.wide_crafted_rows(A)
    n = len(cm)
    v[1:1 + n], r[1:1 + n], m[1:1 + n] = cv, cr, cm
    p = rs.rand(BUCKETS, A).astype(np.float32)
    p[1:1 + n] = cp
    dev = t.visits.device
    t.visits.copy_(torch.from_numpy(v).to(dev))
    t.returns.copy_(torch.from_numpy(r).to(dev))
    t.mask_words.copy_(torch.from_numpy(m.view(np.int64)).to(dev))
    if priors:
        t.priors.copy_(torch.from_numpy(p).to(dev))
    return v, r, m, (p if priors else None)


def lists(rs):
    import test_tree_rule as TRD
    return TRD.lists(rs)


@pytest.mark.parametrize('A', X.TREE_SIZES)
@pytest.mark.parametrize('S_, rows16', [(1, 1), (1, 2), (2, 0), (17, 0), (64, 0)])
def test_the_reweight_stage_alone(S_, rows16, A):
    """Both kernels at S = 1, the 16-lane kernel at S = 2, 17 and 64; lists of 1, 15, 16, 17 and 257; with and without priors; the crafted rows
    of wide_crafted_rows (three slots, ties across them, masks with bits >= 32 alone and with bits at and above A)."""
    v = small_env(A)
    pool, table = v.snapshot(4), v.key_table(BUCKETS // 2)
    assert table.buckets == BUCKETS
    for priors in (False, True):
        t = pool.tree_search(table, 4, 4, c=1.25, q_init=-3.0, priors=priors, spread=S_, rows16=rows16)
        rs = np.random.RandomState(A * 100 + S_)
        vis, ret, m, p = fill(t, A, rs, priors)
        for b in lists(rs):
            marker = rs.rand(BUCKETS, A).astype(np.float32) + 100
            t.rows.copy_(torch.from_numpy(marker).to(t.rows.device))
            v.error_flags()
            t.reweight(b)
            got = t.rows.cpu().numpy()
            named = np.unique(b[(b >= 0) & (b < BUCKETS)])
            exp, bad = spread_rows_reference(vis[named], ret[named], m[named], 1.25, -3.0, S_, None if p is None else p[named])
            assert (got[named].view(np.uint32) == exp.view(np.uint32)).all(), (len(b), named[np.argwhere(got[named] != exp)[:4, 0]], np.argwhere(got[named] != exp)[:4])
            rest = np.ones(BUCKETS, bool)
            rest[named] = False
            assert (got[rest].view(np.uint32) == marker[rest].view(np.uint32)).all(), "a row that was not listed changed"
            assert v.error_flags() == (F_BAD_WEIGHT if bad else 0), (len(b), bad)
        t.close()
    v.close()


@pytest.mark.parametrize('A', X.TREE_SIZES)
def test_one_lane_and_sixteen_lanes_at_spread_1(A):
    v = small_env(A)
    pool, table = v.snapshot(4), v.key_table(BUCKETS // 2)
    out = []
    for rows16 in (2, 1, 0):
        t = pool.tree_search(table, 4, 4, c=1.25, q_init=-3.0, priors=True, rows16=rows16)
        vis, ret, m, p = fill(t, A, np.random.RandomState(A), True)
        t.reweight(np.arange(BUCKETS, dtype=np.int32))
        out.append(t.rows.cpu().numpy().tobytes())
        t.close()
    exp, _ = spread_rows_reference(vis, ret, m, 1.25, -3.0, 1, p)
    assert out[0] == out[1] == out[2] == exp.tobytes() and exp[:, 32:].any()
    v.error_flags()
    v.close()


def tree_make(envs, name, count, spread=1, discount=1.0, **kw):
    spec, v, rows = envs(name)
    pool, table = v.snapshot(N + 8), v.key_table(W.KEYS)
    pool.save()
    t = pool.tree_search(table, count, X.TREE_T, c=X.TREE_C, q_init=X.TREE_Q, spread=spread, discount=discount, **kw)
    m = X.tree_model(name, spread, int(round(discount * 65536)), count, table.buckets)
    return v, pool, table, t, m


@pytest.mark.parametrize('g', [65536, 58982, 0])
def test_the_backup_stage_alone(envs, g):
    """A recorded guided playout of 130 pairs of the A = 48 spec, T = 6, per-pair limits and a bootstrap, against backup_reference."""
    v, pool, table, t0, _ = tree_make(envs, 'w24a48', PAIRS)
    roots = X.tree_roots('w24a48', PAIRS)
    t0.start(roots)
    t0.run(2, SEED)
    rs = np.random.RandomState(6)
    limits = rs.randint(0, X.TREE_T + 1, PAIRS).astype(np.int32)
    boot = rs.randint(-(1 << 30), 1 << 30, PAIRS).astype(np.int32)
    r = pool.playout(roots, X.TREE_T, SEED, first_pair=7 * PAIRS, limits=limits, record=True, path_keys=True, rewards=True, masks=True, table=table,
                     table_weights=t0.rows, device=True)
    rec = {k: getattr(r, k).cpu().numpy() for k in ('actions', 'rewards', 'where', 'depth', 'length')}
    assert (rec['length'] < X.TREE_T).any() and (rec['depth'] >= 1).any() and (rec['actions'] >= 32).any()
    t = pool.tree_search(table, PAIRS, X.TREE_T, c=X.TREE_C, discount=g / 65536)
    t.backup(r, bootstrap=boot)
    vis, ret = np.zeros((table.buckets, v.n_actions), np.int32), np.zeros((table.buckets, v.n_actions), np.int64)
    touched = backup_reference(vis, ret, rec['actions'], rec['rewards'], rec['where'], rec['depth'], rec['length'], None, boot, g)
    assert (t.visits.cpu().numpy() == vis).all() and (t.returns.cpu().numpy() == ret).all()
    assert vis.sum() == (touched >= 0).sum() > 0 and (ret != 0).any() and vis[:, 32:].any(), "something is backed up into a column >= 32"
    assert (t.last['touched'].cpu().numpy()[:X.TREE_T] == touched).all()
    for x in (t, t0, pool, table):
        x.close()


# ------------------------------------------------------------------ h. whole tree runs
@pytest.mark.parametrize('spread, discount', [(1, 1.0), (8, 0.9), (64, 0.5)])
@pytest.mark.parametrize('name', ['w20a33', 'w24a48'])
def test_whole_tree_runs_against_the_model(envs, name, spread, discount):
    v, pool, table, t, m = tree_make(envs, name, N, spread, discount)
    roots = X.tree_roots(name)
    t.start(roots)
    m.start(roots)
    TM.assert_tree(t, table, m, name + ' start', flags=0)
    for i in range(3):
        t.run(1, X.TREE_SEED)
        m.run(1, X.TREE_SEED)
        TM.assert_tree(t, table, m, '%s spread %d discount %s iteration %d' % (name, spread, discount, i), flags=0)
        assert (t.last['actions'].cpu().numpy()[:, :N] == m.last['actions']).all()
    assert any(nd.row[32:].any() for nd in m.node.values()), "no row allots an action >= 32"
    assert v.error_flags() == 0
    for x in (t, pool, table):
        x.close()


# ------------------------------------------------------------------ i. refusals
@pytest.mark.parametrize('field, value', [('n_items', 25), ('n_actions', 49), ('n_recipes', 9)])
def test_create_refuses_what_lies_beyond(field, value):
    cs = W.spec_of('w24a48').compile()
    setattr(cs, field, value)
    h = C.c_void_p()
    rc = _cabi.lib().ngw_create(C.byref(cs), 64, 0, 0, 0, C.byref(h))
    assert rc == _cabi.E_INVALID_ARG and field in _cabi.last_error(), (rc, _cabi.last_error())
