"""The weighted choice among valid actions, host side (no GPU): the rule of include/ngw.h as sample.choose_weighted states it in numpy, held to
the choice written out over the CPU oracle's own Philox (tests/sample_oracle.py); its boundaries, fall-backs and its distribution; the C-ABI
and Python surface; and the forwarding of the adapter, the wrappers and the sharded env on oracle-backed stand-ins."""
import os
import re

import numpy as np
import pytest

import ngw_testlib as T
import sample_oracle as SO
from gym_novel_gridworlds_amd import _cabi, sample
from gym_novel_gridworlds_amd.playout import choose_actions, playout_words
from gym_novel_gridworlds_amd.sample import SAMPLE_TAG, Sampled, bad_weights, choose_weighted, sample_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0x0123456789ABCDEF, (7 << 32) | 5)                                # both halves non-zero
F32 = np.float32
LO, HI = F32(2.0 ** -64), F32(2.0 ** 64)
BELOW_LO, ABOVE_HI = np.nextafter(LO, F32(0)), np.nextafter(HI, F32(np.inf))


def same(got, exp):
    SO.assert_sampled(got, exp, 'choose_weighted')


def test_header_declares_and_library_exports_the_calls():
    raw = open(os.path.join(ROOT, 'include', 'ngw.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    assert re.search(r'\bint\s+ngw_sample_actions\s*\(', text) and re.search(r'\bint\s+ngw_snapshot_playout_weighted\s*\(', text)
    assert re.search(r'#define\s+NGW_SAMPLE_TAG\s+0x53414D50u\b', text) and SAMPLE_TAG == 0x53414D50 == SO.SAMPLE_TAG
    assert re.search(r'#define\s+NGW_F_BAD_WEIGHT\s+16u\b', text) and re.search(r'#define\s+NGW_ABI_VERSION\s+3\b', text)
    from gym_novel_gridworlds_amd.spec import F_BAD_WEIGHT
    assert F_BAD_WEIGHT == 16 == SO.F_BAD_WEIGHT
    L = _cabi.lib()
    for name in ('ngw_sample_actions', 'ngw_snapshot_playout_weighted'):
        assert hasattr(L, name) and name in _cabi.SYMBOLS
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert L.ngw_sample_actions(None, None, None, 0, None, 0, 0, 0, 0, None, None, None) == _cabi.E_INVALID_ARG and 'NULL' in _cabi.last_error()
    assert L.ngw_snapshot_playout_weighted(None, None, None, 0, 1, 0, 0, None, None, None, None, None, None, None, None, None, 0) == _cabi.E_INVALID_ARG


def test_python_surface():
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import PogostickV1Env
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.snapshot import Snapshot
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    for owner in (VecNovelGridworld, ShardedVecNovelGridworld):
        assert callable(owner.sample_actions) and callable(owner.step_sampled), owner
    for owner in (PogostickV1Env, NoveltyWrapper, LimitActions):
        assert callable(owner.sample_action), owner
    assert callable(Snapshot.sample_actions)
    s = Sampled(np.array([1], np.int32), np.array([2.0], F32), np.array([3], np.uint64))
    assert s['mass'] is s.mass and s.action is s[0] and s.mask_words is s[2]


def test_sample_words_equal_the_oracle_generator_under_the_sample_tag():
    pairs = np.array([0, 1, 63, 64, (1 << 32) - 1, 1 << 32, (1 << 63) + 12345, (1 << 64) - 1], np.uint64)
    for seed in SEEDS:
        for t in (0, 3, 4, 7, 1000):
            assert sample_words(seed, pairs, t).tolist() == [SO.philox_word(SAMPLE_TAG, seed, int(p), t) for p in pairs], (hex(seed), t)
    assert (sample_words(SEEDS[0], pairs, 0) != playout_words(SEEDS[0], pairs, 0)).any()           # another tag: another stream


@pytest.mark.parametrize('n_actions', [1, 5, 17, 48])
def test_choose_weighted_equals_the_oracle(n_actions):
    """Random masks (mask 0, every bit and single bits among them) and random weights over 2^-70 .. 2^70 with zeros and bad values; pair
    numbers above 2^32; t on both sides of a Philox block boundary."""
    rs = np.random.RandomState(n_actions)
    every = (1 << n_actions) - 1
    masks = [0, every] + [1 << a for a in range(min(n_actions, 6))] + [int(rs.randint(0, 1 << 30)) * int(rs.randint(0, 1 << 30)) & every for _ in range(60)]
    masks = np.array(masks, np.uint64)
    count = len(masks)
    pairs = np.uint64(1 << 32) * rs.randint(0, 1 << 20, count).astype(np.uint64) + rs.randint(0, 1 << 31, count).astype(np.uint64)
    pairs[:3] = [0, (1 << 32) + 1, (1 << 64) - 1]
    for seed in SEEDS:
        for t, bad in ((0, False), (3, True), (4, False), (7, True)):
            x = SO.random_weights(rs, count, n_actions, bad)
            x[5] = 0                                                                                # a row without any weight: the uniform rule
            got = choose_weighted(masks, x, seed, pairs, t, n_actions)
            same(got, SO.choose(masks, x, seed, pairs, t, n_actions))
            chosen = np.where(masks == 0, np.uint64(every), masks)
            assert (((chosen >> got[0].astype(np.uint64)) & np.uint64(1)) == 1).all()              # a valid action, always
            assert bad_weights(x) == bad == any(SO.is_bad(v) for v in x.reshape(-1))
    # int64 words over the same bits; one weight row for every pair
    x = SO.random_weights(rs, 1, n_actions)[0]
    got = choose_weighted(masks.view(np.int64), x, SEEDS[0], pairs, 4, n_actions)
    same(got, SO.choose(masks, np.tile(x, (count, 1)), SEEDS[0], pairs, 4, n_actions))


def test_rule_3_boundaries():
    """2^-64 and 2^64 count, the floats next to them outside do not; -0.0 and small weights are silently 0; negative, NaN, inf and the float
    above 2^64 raise the flag and count as 0."""
    A, seed = 5, SEEDS[0]
    m = np.array([0b11111], np.uint64)
    one = lambda *x: choose_weighted(m, np.array([x], F32), seed, [9], 2, A)          # noqa: E731
    for kept in (LO, HI, F32(1)):
        a, mass, _ = one(0, 0, kept, 0, 0)
        assert a[0] == 2 and mass[0] == kept and not bad_weights([kept])
    for dropped, flagged in ((BELOW_LO, False), (F32(-0.0), False), (F32(1e-40), False), (ABOVE_HI, True), (F32(-1), True), (F32(np.nan), True),
                             (F32(np.inf), True), (F32(-np.inf), True)):
        x = np.array([[0, 3, dropped, 0, 0]], F32)
        got = choose_weighted(m, x, seed, [9], 2, A)
        assert got[0][0] == 1 and got[1][0] == F32(3) and bad_weights(x) == flagged == SO.is_bad(dropped), dropped
        same(got, SO.choose(m, x, seed, [9], 2, A))
        # alone: no weight is left, the uniform rule on the same word
        x = np.array([[0, 0, dropped, 0, 0]], F32)
        got = choose_weighted(m, x, seed, [9], 2, A)
        assert got[1][0] == 0 and np.signbit(got[1][0]) == np.False_
        same(got, SO.choose(m, x, seed, [9], 2, A))
    # a bad weight on an invalid action raises the flag too (and changes nothing else)
    x = np.array([[1, -5, 1, 1, 1]], F32)
    assert bad_weights(x) and choose_weighted(np.array([0b11101], np.uint64), x, seed, [9], 2, A)[1][0] == 4
    # 48 weights of 2^64: every intermediate stays finite
    big = np.full((1, 48), HI, F32)
    a, mass, _ = choose_weighted(np.array([(1 << 48) - 1], np.uint64), big, seed, [1], 0, 48)
    assert np.isfinite(mass[0]) and mass[0] == F32(48 * 2.0 ** 64)


def test_one_hot_weight_on_an_invalid_action_falls_back_to_the_uniform_rule():
    A, n = 17, 200
    rs = np.random.RandomState(1)
    masks = np.array([int(rs.randint(1, 1 << 17)) & ~(1 << 4) or 1 for _ in range(n)], np.uint64)
    x = np.zeros((n, A), F32)
    x[:, 4] = 7
    pairs = np.arange(n, dtype=np.uint64) + np.uint64(1 << 40)
    a, mass, m = choose_weighted(masks, x, SEEDS[1], pairs, 6, A)
    assert (mass == 0).all() and (m == masks).all()
    # playout.choose_actions fed the same word: its stream differs only by the tag, so choose_weighted is given the playout's words
    pw = playout_words(SEEDS[1], pairs, 6)
    a2, mass2, _ = choose_weighted(masks, x, SEEDS[1], pairs, 6, A, words=pw)
    assert (mass2 == 0).all() and (a2 == choose_actions(masks, SEEDS[1], pairs, 6, A)).all()
    same((a, mass, m), SO.choose(masks, x, SEEDS[1], pairs, 6, A))


def test_an_all_zero_mask_makes_every_action_eligible():
    A = 5
    x = np.array([[0, 0, 0, 0, 3]], F32)
    a, mass, m = choose_weighted(np.array([0], np.uint64), x, 1, [0], 0, A)
    assert a[0] == 4 and mass[0] == 3 and m[0] == 0b11111
    got = choose_weighted(np.zeros(50, np.uint64), np.tile(np.array([1, 2, 3, 4, 5], F32), (50, 1)), 3, np.arange(50), 1, A)
    assert len(set(got[0].tolist())) > 2 and (got[1] == 15).all()
    same(got, SO.choose(np.zeros(50, np.uint64), np.tile(np.array([1, 2, 3, 4, 5], F32), (50, 1)), 3, np.arange(50), 1, A))


def test_the_extreme_words_pick_the_first_and_the_last_weighted_valid_action(monkeypatch):
    """w forced to 0 and to 0xFFFFFFFF through a stubbed word source."""
    A = 17
    mask = np.array([0b10010110001001010], np.uint64)
    x = np.zeros((1, A), F32)
    x[0, [0, 3, 6, 10, 13, 16]] = [5, 0, 2.5, 1e-30, 1e10, 0]          # valid and positive: 6 (3 and 16 are valid but 0; 0 is invalid)
    x[0, 12] = 2.0 ** -70                                            # valid but below 2^-64
    for w, exp in ((0, 6), (0xFFFFFFFF, 13)):
        monkeypatch.setattr(sample, 'sample_words', lambda seed, pairs, t, w=w: np.full(np.shape(pairs), w, np.uint32))
        a, mass, _ = choose_weighted(mask, x, 1, [0], 0, A)
        assert a[0] == exp and mass[0] > 0, (w, a)
        assert SO.select(int(mask[0]), x[0], w, A)[0] == exp
    # a tiny weight behind a huge one is never reached by c[a] > thr alone, and is not the answer to w = 0xFFFFFFFF unless it is last
    monkeypatch.setattr(sample, 'sample_words', lambda seed, pairs, t: np.full(np.shape(pairs), 0xFFFFFFFF, np.uint32))
    y = np.array([[2.0 ** 40, 2.0 ** -40, 0]], F32)
    assert choose_weighted(np.array([0b111], np.uint64), y, 1, [0], 0, 3)[0][0] == 0 == SO.select(0b111, y[0], 0xFFFFFFFF, 3)[0]


def test_contract_sanity_the_shares_follow_the_weights():
    """120 000 pairs on one mask with 6 valid actions and weights 1 : 2 : 3 : 4 : 5 : 6 at a fixed seed (deterministic): the chi-square of the
    counts, 5 degrees of freedom, stays below 20.5, the 0.999 quantile.  With seed 0x0123456789ABCDEF the statistic is 6.119 (counts 5642,
    11274, 17010, 23025, 28723, 34326 against expectations 5714.3 .. 34285.7); nothing outside the mask is drawn."""
    A, n = 17, 120000
    valid = [1, 3, 6, 10, 13, 16]
    mask = sum(1 << a for a in valid)
    x = np.full(A, 9, F32)                                           # (weights on invalid actions do not matter)
    x[valid] = [1, 2, 3, 4, 5, 6]
    a, mass, _ = choose_weighted(np.full(n, mask, np.uint64), x, SEEDS[0], np.arange(n, dtype=np.uint64), 0, A)
    counts = np.bincount(a, minlength=A)
    assert (mass == 21).all() and counts.sum() == n and counts[[i for i in range(A) if i not in valid]].sum() == 0
    expected = n * np.arange(1, 7) / 21.0
    chi2 = float((((counts[valid] - expected) ** 2) / expected).sum())
    print('chi2 = %.3f, counts = %s' % (chi2, counts[valid].tolist()))
    assert chi2 < 20.5, (chi2, counts[valid])


def test_choose_weighted_refuses_bad_arguments():
    x = np.ones((1, 5), F32)
    with pytest.raises(ValueError, match='n_actions'):
        choose_weighted([1], x, 1, [0], 0, 49)
    with pytest.raises(ValueError, match='at or above n_actions'):
        choose_weighted([1 << 5], x, 1, [0], 0, 5)
    with pytest.raises(ValueError, match='float32'):
        choose_weighted([1], x.astype(np.float64), 1, [0], 0, 5)
    with pytest.raises(ValueError, match='float32'):
        choose_weighted([1], np.ones((2, 5), F32), 1, [0], 0, 5)
    with pytest.raises(ValueError, match='numbered from 0'):
        choose_weighted([1], x, 1, [0], -1, 5)
    for bad in ((-1, 0, 0), (1 << 64, 0, 0), (0, -1, 0), (0, 0, 1 << 32), (0, 0, -1)):
        with pytest.raises(ValueError, match='outside'):
            sample.check_seed(*bad)
    assert sample.check_seed(np.int64(5), 0, np.int32(3)) == (5, 0, 3)


def _adapter(monkeypatch, cfg='axe10'):
    monkeypatch.setattr(T, 'OracleVec', SO.OracleVecSample)          # (make_adapter_env's oracle backend, with the sampling calls)
    env = T.make_adapter_env(cfg, backend='oracle')
    env.reset()
    for a in (0, 1, 0, 2, 0):
        env.step(a)
    return env


def test_adapter_and_wrappers_forward_sample_action_and_weighted_playouts(monkeypatch):
    """The single-env adapter under a novelty wrapper on the oracle-backed stand-in: Python scalars, the oracle's for its state; playouts
    forward `weights`; LimitActions checks its weights' shape against its own list before anything runs."""
    from gym_novel_gridworlds_amd.wrappers import LimitActions
    env = _adapter(monkeypatch)
    vec = env.unwrapped._backend()
    A = vec.n_actions
    x = SO.random_weights(np.random.RandomState(4), 1, A)[0]
    x[0] = 1
    got = env.sample_action(x, SEEDS[0], t=5)
    exp = SO.oracle_sample(vec.spec, vec.o.st, [0], x[None], SEEDS[0], 0, 5)
    assert got == (int(exp[0][0]), float(exp[1][0]), int(exp[2][0])) and [type(v) for v in got] == [int, float, int]
    assert got == env.unwrapped.sample_action(x, SEEDS[0], t=5)
    play = env.playouts(6, 4, SEEDS[1], weights=x)
    _, rep, _, _ = SO.oracle_weighted_playout(vec.spec, vec.o.st, np.zeros(6, np.int64), 4, SEEDS[1], x)
    for k in ('ret', 'length', 'ended', 'info', 'first_action'):
        assert (play[k] == rep[k]).all(), k
    plain = env.playouts(6, 4, SEEDS[1])
    _, rep0, _, _ = SO.PO.oracle_playout(vec.spec, vec.o.st, np.zeros(6, np.int64), 4, SEEDS[1])
    assert (plain.first_action == rep0['first_action']).all()
    lim = LimitActions(env, {'Forward', 'Break'})
    for bad in (x, np.ones(3, F32), np.ones((1, 2), F32)):
        with pytest.raises(ValueError, match='one weight per limited action'):
            lim.sample_action(bad, 1)


def test_sharded_env_forwards_to_its_shard():
    spec = T.build_spec('pogo10')
    sh = SO.sharded_on_oracle(spec=spec, global_num_envs=6, seed=SO.XO.good_seed(spec, 6))
    sh.reset()
    x = SO.random_weights(np.random.RandomState(2), 6, sh.local.n_actions)
    got = sh.sample_actions(x, SEEDS[0], t=3)
    SO.assert_sampled(got, SO.oracle_sample(spec, sh.local.o.st, np.arange(6), x, SEEDS[0], sh.first, 3), 'shard')
    got = sh.sample_actions(x[[4, 1]], SEEDS[0], envs=[4, 1])
    SO.assert_sampled(got, SO.oracle_sample(spec, sh.local.o.st, [4, 1], x[[4, 1]], SEEDS[0], sh.first, 0), 'shard, envs')
    assert sh.playouts(2, 3, SEEDS[0], weights=x[0]).ret.shape == (6, 2)


def test_host_argument_checks_refuse_before_any_device_call():
    """check_weights on the CPU device: shapes, dtypes, the transpose of a host array, a tensor used in place."""
    import torch
    cpu = torch.device('cpu')
    x = np.arange(6, dtype=np.float64).reshape(2, 3)
    t, mine = sample.check_weights(x, 2, 3, cpu)
    assert mine and t.dtype == torch.float32 and tuple(t.shape) == (3, 2) and t.is_contiguous() and t.numpy().tolist() == x.T.tolist()
    t, mine = sample.check_weights([1, 2, 3], 7, 3, cpu, per_pair=False)
    assert mine and tuple(t.shape) == (3,)
    own = torch.ones(3, 2)
    assert sample.check_weights(own, 2, 3, cpu) == (own, False)
    bad_values = np.array([[np.nan, -1, np.inf], [1e300, 0, 1]])                   # values are the device's to report: never refused here
    assert sample.check_weights(bad_values, 2, 3, cpu)[0].shape == (3, 2)
    for bad in (np.ones((3, 2)), np.ones(3), np.ones((2, 3, 1)), np.ones((2, 4))):
        with pytest.raises(ValueError, match='shape'):
            sample.check_weights(bad, 2, 3, cpu)
    for bad in (np.ones((2, 3), bool), np.ones((2, 3), np.float16), np.ones((2, 3), complex), np.array([['a'] * 3] * 2)):
        with pytest.raises(ValueError, match='dtype'):
            sample.check_weights(bad, 2, 3, cpu)
    for bad in (torch.ones(2, 3), torch.ones(3, 2, dtype=torch.float64), torch.ones(2, 3).T, torch.ones(3)):
        with pytest.raises(ValueError, match='contiguous float32 tensor'):
            sample.check_weights(bad, 2, 3, cpu)
