"""Action masks on the MI355X (csrc/ngw_mask.inc, include/ngw.h ngw_set_action_mask ...), held to the CPU oracle: the expected mask of a
state is what the unmodified oracle reports as `result` when each action is stepped from a copy of it (tests/mask_oracle.py)."""
import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
from gym_novel_gridworlds_amd import VecNovelGridworld
from gym_novel_gridworlds_amd.spec import make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_G4 = sorted(T.spec_json()['cfgs'])


def load_state(v, st):
    v.set_state(0, map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)


def assert_masks(v, spec, st, where):
    exp = M.oracle_mask_words(spec, st)
    got = v.action_mask_words().copy()
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, "%s: %d envs differ, first env %d: got %x expected %x" % (where, len(bad), bad[0], int(got[bad[0]]), int(exp[bad[0]]))


@pytest.mark.parametrize('cfg', CFG_G4)
def test_masks_pinned_to_reference_single_steps(cfg):
    """1 + 2: every G4 pre-state: bit ss_action is the reference's ss_result, and the whole mask is the oracle's; then, from states of
    seeded random play, the standalone and the fused (masks on) forms both equal the oracle's."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    v = VecNovelGridworld(spec=spec, num_envs=st.n, seed=1)
    load_state(v, st)
    words = v.action_mask_words().copy()
    bit = (words >> g['ss_action'].astype(np.uint64)) & np.uint64(1)
    assert (bit == g['ss_result'].astype(np.uint64)).all()
    assert_masks(v, spec, st, cfg + ' G4')
    v.close()
    # seeded random play: standalone (masks off) and fused (masks on) forms
    n, A = 515, len(spec.actions_id)
    seed = next(sd for sd in range(4, 40) if not Oracle(spec.compile(), n, seed=sd).reset() & 2)   # (tight maps can exhaust the placement)
    for on in (False, True):
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
        o = Oracle(spec.compile(), n, seed=seed)
        v.set_action_masks(on)
        v.reset(); o.reset()
        rs = np.random.RandomState(5)
        for t in range(40):
            a = rs.randint(0, A, n).astype(np.int32)
            v.step(a); o.step(a)
            if t % 8 == 7:
                assert_masks(v, spec, o.st, '%s random play t=%d masks_on=%d' % (cfg, t, on))
        v.close()


TRAJ = [('pogo10', None, 'auto'), ('pogo10', None, 0), ('bow20', None, 'auto'), ('add32', None, 'auto'), ('add32', None, 0),
        ('pogo64', 64, 'auto'), ('pogo64', 64, 0), ('fencer10m', None, 'auto'), ('fencer12h', None, 0), ('crate12h', None, 'auto'),
        ('fire10h', None, 'auto'), ('stk_crate_fr12', None, 0), ('stk_fr_crate12', None, 'auto'), ('stk_fen_fire12', None, 'auto'),
        ('fencer24h', None, 'auto')]


@pytest.mark.parametrize('cfg,S,prefetch,fused', [t + (1,) for t in TRAJ] + [('pogo10', None, 'auto', 0), ('add32', None, 0, 0),
                                                                           ('stk_fr_crate12', None, 'auto', 0)])
def test_fused_masks_along_trajectories(cfg, S, prefetch, fused, monkeypatch):
    """3: masks on, random actions, 4 099 envs (a partial last wave), autoreset from prepared episodes ('auto') and inline (0): after every
    step the mask is the oracle's mask of the post-step state, and each step's result is the previous mask's bit of the chosen action.
    fused = 1: the step kernel computes the masks itself (ngw_step_lean<..., MASK>); 0: the standalone kernel behind every step."""
    monkeypatch.setenv('NGW_MASK_FUSED', str(fused))
    spec = make_spec(T.POGO, 64) if cfg == 'pogo64' else T.build_spec(cfg)
    n, A = 4099, len(spec.actions_id)
    H = 12 if spec.map_size <= 12 else 25
    steps = 60 if spec.map_size >= 32 else 150
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=17, autoreset=True, horizon=H, reset_prefetch=prefetch)
    o = Oracle(spec.compile(), n, seed=17, autoreset=True, horizon=H)
    v.set_action_masks(True)
    v.reset(); o.reset()
    prev = v.action_mask_words().copy()
    assert_masks(v, spec, o.st, cfg + ' after reset')
    rs = np.random.RandomState(23)
    for t in range(steps):
        a = rs.randint(0, A, n).astype(np.int32)
        if o.step(a) & 2:                                       # a tight map exhausted the placement of an autoreset: both sides raise
            with pytest.raises(AssertionError):
                v.step(a)
            break
        _, reward, done, info = v.step(a)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        exp_res = ((prev >> a.astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert (info['result'] == exp_res).all(), "step %d: result differs from the previous mask's bit" % t
        prev = v.action_mask_words().copy()
        assert_masks(v, spec, o.st, '%s step %d' % (cfg, t))
    assert v.error_flags() == 0
    v.close()


def test_masks_change_nothing_else_and_graphs_capture_them():
    """4: same seed, masks on vs off: identical state and outputs after every step; a graph built with masks on replays to the same masks
    as eager steps."""
    import torch
    spec = T.build_spec('fencer10m')
    n, A = 3000, len(spec.actions_id)
    a = VecNovelGridworld(spec=spec, num_envs=n, seed=21, autoreset=True, horizon=7)
    b = VecNovelGridworld(spec=spec, num_envs=n, seed=21, autoreset=True, horizon=7)
    a.set_action_masks(True)
    a.reset(); b.reset()
    rs = np.random.RandomState(2)
    for t in range(50):
        act = rs.randint(0, A, n).astype(np.int32)
        _, ra, da, ia = a.step(act, copy=True)
        _, rb, db, ib = b.step(act, copy=True)
        assert (ra == rb).all() and (da == db).all(), t
        for k in ('result', 'step_cost_code', 'message_code', 'message_arg'):
            assert (np.asarray(ia[k]) == np.asarray(ib[k])).all(), (t, k)
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert (sa[k] == sb[k]).all(), (t, k)
    acts = torch.randint(0, A, (6, n), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    a.graph_build(acts.data_ptr(), n, 6)
    a.graph_launch(2)
    for rep in range(2):
        for t in range(6):
            b.step_device(acts[t].data_ptr())
    wa = a.action_mask_words().copy()
    wb = b.action_mask_words().copy()
    assert (wa == wb).all()
    o = M.state_from(spec, *[b.get_state()[k] for k in ('map', 'loc', 'facing', 'inv', 'selected')])
    assert (wa == M.oracle_mask_words(spec, o)).all()
    assert a.error_flags() == 0 and b.error_flags() == 0
    a.close(); b.close()


@pytest.mark.parametrize('on', [False, True])
def test_masks_follow_resets_state_injection_novelties_and_rollouts(on):
    """5: after reset(mask), set_state, inject_novelty (axe adds a Select column, axetobreak changes Break) and a rollout, action_masks()
    is the oracle's."""
    spec = T.build_spec('pogo10')
    n = 700
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=8, autoreset=True, horizon=20)
    o = Oracle(spec.compile(), n, seed=8, autoreset=True, horizon=20)
    v.set_action_masks(on)
    v.reset(); o.reset()
    rs = np.random.RandomState(1)
    A = len(spec.actions_id)
    for t in range(10):
        act = rs.randint(0, A, n).astype(np.int32)
        v.step(act); o.step(act)
    m = (rs.rand(n) < 0.4).astype(np.uint8)
    v.reset(m); o.reset(m)
    assert (v.action_masks() == M.oracle_masks(spec, o.st)).all()
    inv = rs.randint(0, 4, (n, len(spec.items_id))).astype(np.int32)
    v.set_state(0, inv=inv); o.st.inv[...] = inv
    assert (v.action_masks() == M.oracle_masks(spec, o.st)).all()
    v.rollout(13, action_seed=5); o.rollout(13, 5, 0)
    assert (v.action_masks() == M.oracle_masks(spec, o.st)).all()
    for nov in [('axe', 'medium', 'wooden', ''), ('axetobreak', 'hard', 'wooden', '')]:
        import copy
        from gym_novel_gridworlds_amd.novelty import apply_novelty
        spec2 = copy.deepcopy(v.spec)
        apply_novelty(spec2, *nov)
        v.rebuild(spec2)
        assert v.n_actions == len(spec2.actions_id)
        v.reset()
        st = v.get_state()
        o = M.state_from(spec2, st['map'], st['loc'], st['facing'], st['inv'], st['selected'])
        got = v.action_masks()
        assert got.shape == (n, len(spec2.actions_id))
        assert (got == M.oracle_masks(spec2, o)).all(), nov
        inv = rs.randint(0, 3, (n, len(spec2.items_id))).astype(np.int32)
        sel = rs.randint(0, len(spec2.items_id), n).astype(np.int32)
        v.set_state(0, inv=inv, selected=sel)
        o.inv[...] = inv; o.selected[...] = sel
        assert (v.action_masks() == M.oracle_masks(spec2, o)).all(), nov
        spec = spec2
    v.close()


def _adapter_oracle_mask(env):
    """The oracle's mask of the adapter's current state (its public attributes)."""
    base = env
    while hasattr(base, 'env') and not hasattr(base, '_backend'):
        base = base.env
    spec = base._sync_spec()
    st = base._backend().get_state()
    return M.oracle_masks(spec, M.state_from(spec, st['map'], st['loc'], st['facing'], st['inv'], st['selected']))[0]


def test_single_env_masks_in_the_reference_loop_shape_and_no_relaunch():
    """6: tests/random_action.py's loop shape (reset every ten steps), bare and wrapped in LimitActions: action_masks() before every step()
    is the oracle's; the calls start no resident step loop of their own."""
    import gym_novel_gridworlds_amd as G
    from gym_novel_gridworlds_amd import _cabi
    import ctypes as C
    L = _cabi.lib()
    L.ngw_debug_solo_starts.restype = C.c_longlong
    L.ngw_debug_solo_starts.argtypes = [C.c_void_p]
    np.random.seed(0)
    env = G.make('NovelGridworld-Pogostick-v1')
    env.reset()
    checked = 0
    for i in range(60):
        vec = env._backend()
        s0 = L.ngw_debug_solo_starts(vec._h)
        mask = env.action_masks()
        assert L.ngw_debug_solo_starts(vec._h) == s0, "action_masks() relaunched the resident loop at step %d" % i
        exp = _adapter_oracle_mask(env)
        assert mask.dtype == np.bool_ and (mask == exp).all(), i
        a = env.action_space.sample()
        obs, reward, done, info = env.step(a)
        assert info['result'] == bool(mask[a]), i
        checked += 1
        if (i + 1) % 10 == 0:
            env.map_size = int(np.random.randint(low=10, high=20, size=1)[0])
            env.reset()
    # a tight step loop: masks read from the loop's speculated records, no relaunch between one reset and the next
    env.reset()
    vec = env._backend()
    starts = None
    rs = np.random.RandomState(4)
    for i in range(200):
        mask = env.action_masks()
        a = int(rs.randint(0, len(mask)))
        _, _, _, info = env.step(a)
        assert info['result'] == bool(mask[a]), i
        if i == 5:
            starts = L.ngw_debug_solo_starts(vec._h)
    assert L.ngw_debug_solo_starts(vec._h) - starts <= 2          # (only the loop's own idle-limit endings may restart it)
    # LimitActions: the mask in the limited id space
    limited = {'Forward', 'Left', 'Right', 'Break', 'Craft_plank', 'Craft_stick'}
    w = G.LimitActions(G.make('NovelGridworld-Pogostick-v1'), limited)
    w.reset()
    names = sorted(limited)
    for i in range(40):
        mask = w.action_masks()
        full = _adapter_oracle_mask(w)
        exp = np.array([full[w.actions_id[nm]] for nm in names])
        assert mask.shape == (len(limited),) and (mask == exp).all(), i
        a = int(np.random.randint(0, len(limited)))
        _, _, _, info = w.step(a)
        assert info['result'] == bool(mask[a]), i
        if (i + 1) % 10 == 0:
            w.reset()
    env.close(); w.close()


def test_torch_view_and_sharded_masks():
    """7: action_masks(device=True) equals the host array; the sharded env's masks are the matching slice of one unsharded handle."""
    import torch
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    spec = T.build_spec('axe10')
    n = 2048
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=9, autoreset=True, horizon=20)
    v.reset()
    v.rollout(17, action_seed=3)
    host = v.action_masks()
    dev = v.action_masks(device=True)
    assert dev.dtype == torch.bool and dev.device.type == 'cuda' and tuple(dev.shape) == host.shape
    assert (dev.cpu().numpy() == host).all()
    assert (v.action_mask_words(device=True).cpu().numpy().view(np.uint64) == v.action_mask_words()).all()
    sh = ShardedVecNovelGridworld(global_num_envs=n, spec=spec, seed=9, autoreset=True, horizon=20)
    sh.reset()
    sh.rollout(17, action_seed=3)
    lo = sh.local.env_index_base
    assert (sh.action_masks() == host[lo:lo + sh.num_envs]).all()
    v.close(); sh.close()


def test_masks_after_multi_step_calls_and_with_the_fused_lidar():
    """The masks after ngw_step_device_many (computed for its last step only) and with the fused LidarInFront observation on (the standalone
    kernel behind the bit-row lidar step) are the oracle's."""
    import torch
    from gym_novel_gridworlds_amd import LidarInFront
    spec = T.build_spec('pogo10')
    n, A = 1500, len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=12, autoreset=True, horizon=9)
    o = Oracle(spec.compile(), n, seed=12, autoreset=True, horizon=9)
    v.set_action_masks(True)
    v.reset(); o.reset()
    acts = np.random.RandomState(3).randint(0, A, (7, n)).astype(np.int32)
    ad = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()
    v.step_device_many(ad.data_ptr(), n, 7)
    for t in range(7):
        o.step(acts[t])
    assert_masks(v, spec, o.st, 'after step_device_many')
    w = LidarInFront(v, num_beams=8)
    rs = np.random.RandomState(4)
    for t in range(30):
        a = rs.randint(0, A, n).astype(np.int32)
        w.step(a); o.step(a)
        assert_masks(v, spec, o.st, 'fused lidar step %d' % t)
    v.close()
