"""One-env handles (the gym.Env adapter, BASELINE config 1) run a resident step loop (csrc/ngw_solo.inc): while it runs, the state in
HBM is correct only once the loop has committed the last posted action, and the handle's stream is busy until the loop ends.  Every
other C-ABI entry point ends the loop first (ngw_host.h, solo_stop; tests/test_solo_stop_audit.py checks the sources).  Here the entry
points meet a RUNNING loop, and everything they return is held to the CPU oracle element by element:
  (a) the wrapped adapter (LidarInFront / AgentMap + a novelty on top) stepping freely - no state injection - against an oracle-backed twin;
  (b) a random sequence of C-ABI calls between step1() calls, under idle limits that make the loop end near the host's step period;
  (c) every entry point reachable from Python, called right behind a step under a 2 s idle limit: it must return at once."""
import ctypes as C
import time

import numpy as np
import pytest

import ngw_testlib as T

pytestmark = pytest.mark.gpu


def _solo_starts(vec):
    from gym_novel_gridworlds_amd import _cabi
    f = _cabi.lib().ngw_debug_solo_starts
    f.argtypes, f.restype = [C.c_void_p], C.c_longlong
    return int(f(vec._h))


def _outcome(fn):
    """fn()'s value, or the exception it raised as (type, message): both sides of a comparison must fail alike (a placement that
    cannot succeed raises AssertionError on the device and on the oracle)."""
    try:
        return fn()
    except (AssertionError, ValueError) as e:
        return ('raised', type(e).__name__, str(e))


# ------------------------------------------------------------------------------------------------ (a) free-running wrapped adapter
def _wrapped_adapter(cfg, backend, wrap):
    import gym_novel_gridworlds_amd as G
    env_id, S, nov = T.CFGS[cfg]
    env = G.make(env_id)
    if backend == 'oracle':
        env._make_backend = lambda spec, seed_: T.OracleVec(spec, 1, seed=seed_)
    env.seed(9)
    env.map_size = S
    env = G.LidarInFront(env, num_beams=8) if wrap == 'lidar' else G.AgentMap(env)      # observation wrapper first ...
    for one in T.novelty_list(nov):
        env = G.inject_novelty(env, *one)                                                # ... novelty on top (tests/random_action.py:24-42)
    return env


def _same_obs(a, b):
    if isinstance(a, tuple) or isinstance(b, tuple):
        return type(a) is type(b) and len(a) == len(b) and all(_same_obs(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_obs(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and (a == b).all()
    return a == b


@pytest.mark.parametrize('wrap', ['lidar', 'agentmap'])
@pytest.mark.parametrize('cfg', ['pogo10', 'bow20', 'axe10', 'fire10h', 'add12m', 'pogo13'])
def test_free_running_wrapped_adapter_matches_oracle_twin(cfg, wrap):
    """The reference's own loop (tests/random_action.py:51-64): random actions, a new map_size and reset() every 10 steps, an observation
    wrapper computing every observation on the device right behind the step the loop has just served."""
    from mask_oracle import oracle_masks
    hip, twin = _wrapped_adapter(cfg, 'hip', wrap), _wrapped_adapter(cfg, 'oracle', wrap)
    S = T.CFGS[cfg][1]
    rs = np.random.RandomState(sum(map(ord, cfg + wrap)))
    oh, ot = _outcome(hip.reset), _outcome(twin.reset)
    assert _same_obs(oh, ot), (cfg, 'reset')
    n_steps, n_masks = 80, 0
    A = len(hip.unwrapped.actions_id)
    for t in range(n_steps):
        a = int(rs.randint(0, A))
        gh, gt = _outcome(lambda: hip.step(a)), _outcome(lambda: twin.step(a))
        assert _same_obs(gh, gt), (cfg, wrap, t, a)
        if t % 4 == 3:
            got = hip.unwrapped.action_masks()
            vec = twin.unwrapped._backend()
            assert (got == oracle_masks(vec.spec, vec.o.st)[0]).all(), (cfg, wrap, t, 'action_masks')
            n_masks += 1
        if (t + 1) % 10 == 0:
            size = S if (t + 1) % 20 == 0 else int(rs.randint(10, 21))
            hip.unwrapped.map_size = twin.unwrapped.map_size = size
            oh, ot = _outcome(hip.reset), _outcome(twin.reset)
            assert _same_obs(oh, ot), (cfg, wrap, t, 'reset', size)
    starts = sum(_solo_starts(v) for v in hip.unwrapped._vec_cache.values())
    assert starts >= n_steps // 2, "the resident loop served %d launches for %d steps" % (starts, n_steps)
    assert n_masks == n_steps // 4
    hip.close()


# ------------------------------------------------------------------------------------------------ (b) C-ABI call-sequence fuzz
@pytest.mark.parametrize('timeout_us', ['', '0', '3', '8', '20'])
@pytest.mark.parametrize('cfg', ['pogo10', 'bow20', 'fire10h', 'add12m'])
def test_entry_points_between_loop_steps_match_oracle(cfg, timeout_us, monkeypatch):
    import torch
    import gym_novel_gridworlds_amd as G
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    from oracle.ngw_oracle import Oracle, lidar, agent_view
    from mask_oracle import oracle_masks
    if timeout_us:
        monkeypatch.setenv('NGW_SOLO_TIMEOUT_US', timeout_us)
    else:
        monkeypatch.delenv('NGW_SOLO_TIMEOUT_US', raising=False)
    spec = T.build_spec(cfg)
    A, S, K = len(spec.actions_id), spec.map_size, len(spec.items_id)
    seed = 17 + len(timeout_us) * 31 + sum(map(ord, cfg))
    v = G.VecNovelGridworld(spec=spec, num_envs=1, seed=seed)
    o = Oracle(spec.compile(), 1, seed=seed)
    rs = np.random.RandomState(seed)
    lid = None                                              # (config, compiled config, fused) of the configured lidar
    outs_valid = [False]                                    # the device's reward / done / info words are the last step's

    def same_state(where):
        mb, r, c, f, ib, sel, steps = v.last_state1()
        assert (np.frombuffer(mb, np.int8) == o.st.map[0]).all() and (r, c, f) == (o.st.loc[0][0], o.st.loc[0][1], o.st.facing[0]), where
        assert (np.frombuffer(ib, np.int32) == o.st.inv[0]).all() and sel == o.st.selected[0] and steps == o.st.step_count[0], where

    def same_device_state(where):
        st = v.get_state()
        for k, want in (('map', o.st.map), ('loc', o.st.loc), ('facing', o.st.facing), ('inv', o.st.inv), ('selected', o.st.selected),
                        ('step_count', o.st.step_count)):
            assert (st[k] == want).all(), (where, k)

    def check_lidar(where):
        lc, cc, _ = lid
        got = v.lidar_observation()
        got = v.lidar_widen(got) if isinstance(got, tuple) else got
        assert (got == lidar(cc, S, K, o.st.map, o.st.loc, o.st.facing, o.st.inv)).all(), where

    def reset_both():
        got = _outcome(v.reset1)
        assert (got is not None) == bool(o.reset() & 2), got       # (bit 2 of the oracle's flags: a placement that cannot succeed)

    reset_both()
    for t in range(110):
        a = int(rs.randint(0, A))
        got = v.step1(a); o.step(np.array([a], np.int32))
        outs_valid[0] = True
        exp = (int(o.reward[0]), bool(o.done[0]), bool(o.result[0]), int(o.cost_code[0]), int(o.msg_code[0]), int(o.msg_arg[0]))
        assert got == exp, (t, a, got, exp)
        same_state(t)
        if lid is not None and lid[2]:
            check_lidar((t, 'fused lidar after the step'))
        k = rs.randint(0, 20)
        where = (t, k)
        if k == 0:                                          # lidar: a row format, fused or not (switching between the two)
            lc = LidarConfig(spec, int(rs.choice([8, 5])))
            fused = bool(rs.randint(0, 2))
            v.lidar_configure(lc, fused=fused, dtype=[np.int32, np.int16, 'packed'][rs.randint(0, 3)])
            lid = (lc, lc.compile(spec), fused)
            if not fused:                                   # (a fused observation is made by the next step / reset launch)
                check_lidar(where)
        elif k == 1 and lid is not None and not lid[2]:
            check_lidar(where)
        elif k == 2:                                        # AgentMap windows, host copy and device view
            vs = int(rs.choice([1, 5, 12]))
            want = agent_view(o.st.map, o.st.loc, vs)
            assert (v.agent_view(vs, copy=True) == want).all(), (where, vs)
            assert (v.agent_view(vs, device=True).cpu().numpy() == want).all(), (where, vs, 'device')
        elif k == 3:
            assert (v.action_masks() == oracle_masks(spec, o.st)).all(), where
        elif k == 4:                                        # terminal capture on / off (on: steps take a launch each, no loop)
            v.set_terminal_capture(bool(rs.randint(0, 2)))
            if v.terminal_capture:
                v.terminal_observation()
        elif k == 5:                                        # fused rollout with the episode accumulators, against the oracle stepped one by one
            if o.done[0]:
                reset_both()
            v.rollout_outputs(accumulate=True)
            n, aseed, t0 = int(rs.randint(1, 9)), int(rs.randint(0, 1 << 30)), int(rs.randint(0, 1000))
            v.rollout(n, action_seed=aseed, t0=t0)
            run_ret = run_len = sum_ret = n_eps = 0
            for i in range(n):
                o.rollout(1, aseed, t0 + i)
                run_ret += int(o.reward[0]); run_len += 1
                if o.done[0]:
                    sum_ret += run_ret; n_eps += 1; run_ret = run_len = 0
            stt = v.episode_stats(clear=True)
            assert (stt['run_return'][0], stt['run_length'][0], stt['sum_return'][0], stt['n_episodes'][0]) == (run_ret, run_len, sum_ret, n_eps), where
            same_device_state(where)
            v.rollout_outputs()
            outs_valid[0] = True
        elif k == 6:
            v.set_reset_prefetch(int(rs.choice([0, 1, 4, 1 << 20])))
        elif k == 7:
            v.set_reset_prefetch_depth(int(rs.choice([0, 1, 2, 4, 8])))
        elif k == 8:                                        # the multi-GPU payload: packed on the device, unpacked again
            offs = v.pack_layout()
            payload = torch.zeros(offs[7], dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            v.pack_obs(payload.data_ptr())
            v.sync()
            p = payload.cpu().numpy()
            sec = lambda i, dt: p[offs[i]:offs[i + 1]].view(np.uint8)[:np.dtype(dt).itemsize * {0: S * S, 1: 2, 2: 1, 3: K, 4: 1, 5: 1, 6: 1}[i]].view(dt)
            assert (sec(0, np.int8) == o.st.map[0]).all() and (sec(1, np.int32) == o.st.loc[0]).all(), where
            assert sec(2, np.int32)[0] == o.st.facing[0] and (sec(3, np.int32) == o.st.inv[0]).all(), where
            if outs_valid[0]:
                assert sec(4, np.int32)[0] == o.reward[0] and sec(5, np.uint8)[0] == o.done[0] and sec(6, np.uint32)[0] == o.info[0], where
        elif k == 9:                                        # a torch stream ordered behind the handle's: the device views read there
            s = torch.cuda.Stream()
            v.stream_order(s.cuda_stream, False)
            with torch.cuda.stream(s):
                dev = {name: x.clone() for name, x in v.device_observation().items()}
            s.synchronize()
            assert (dev['map'].cpu().numpy().reshape(-1) == o.st.map[0]).all(), where
            assert (dev['agent_location'].cpu().numpy() == o.st.loc).all() and (dev['agent_facing_id'].cpu().numpy() == o.st.facing).all(), where
            assert (dev['inventory_items_quantity'].cpu().numpy() == o.st.inv).all(), where
        elif k == 10:
            time.sleep(0.002)                               # past every idle limit here
        elif k == 11 or (o.done[0] and k < 15):
            reset_both()
            outs_valid[0] = False
            same_state((t, 'reset'))
            if lid is not None:
                check_lidar((t, 'lidar after the reset'))
    same_device_state('end')
    assert v.error_flags() == 0
    v.close()


# ------------------------------------------------------------------------------------------------ (c) prompt return behind a running loop
def test_entry_points_return_promptly_behind_a_running_loop(monkeypatch):
    """A 2 s idle limit: an entry point that queued its work behind the running loop instead of ending it would wait ~2 s.  Each call
    follows a step1() that (re)started the loop, returns within 0.25 s, and what it returns equals the oracle."""
    import torch
    import gym_novel_gridworlds_amd as G
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    from oracle.ngw_oracle import Oracle, lidar, agent_view
    monkeypatch.setenv('NGW_SOLO_TIMEOUT_US', '2000000')              # (100 ticks per us: 2e8 ticks fit the 32-bit limit)
    spec = T.build_spec('pogo10')
    A, S, K = len(spec.actions_id), spec.map_size, len(spec.items_id)
    v = G.VecNovelGridworld(spec=spec, num_envs=1, seed=23)
    o = Oracle(spec.compile(), 1, seed=23)
    v.reset1(); o.reset()
    rs = np.random.RandomState(23)
    lc = LidarConfig(spec, 8)
    cc = lc.compile(spec)
    LIMIT = 0.25

    def step():
        s0 = _solo_starts(v)
        a = int(rs.randint(0, A))
        v.step1(a); o.step(np.array([a], np.int32))
        assert _solo_starts(v) == s0 + 1, "the step did not start the loop: the call after it would not meet a running one"

    def timed(name, fn):
        step()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        assert dt < LIMIT, "%s waited %.3f s behind the running loop" % (name, dt)
        return out

    def state_ok(name):
        st = v.get_state()
        assert (st['map'] == o.st.map).all() and (st['loc'] == o.st.loc).all() and (st['inv'] == o.st.inv).all(), name

    want_lidar = lambda: lidar(cc, S, K, o.st.map, o.st.loc, o.st.facing, o.st.inv)
    timed('lidar_configure', lambda: v.lidar_configure(lc, fused=False, dtype=np.int32))          # ngw_lidar_configure, _set_output, _fuse
    assert (timed('lidar_observation', v.lidar_observation) == want_lidar()).all()                   # ngw_lidar + ngw_get_lidar
    assert (timed('agent_view', lambda: v.agent_view(5, copy=True)) == agent_view(o.st.map, o.st.loc, 5)).all()
    assert (timed('agent_view device', lambda: v.agent_view(3, device=True)).cpu().numpy() == agent_view(o.st.map, o.st.loc, 3)).all()
    timed('set_reset_prefetch', lambda: v.set_reset_prefetch(4))
    timed('set_reset_prefetch_depth', lambda: v.set_reset_prefetch_depth(2))
    timed('rollout_outputs', lambda: v.rollout_outputs(accumulate=True))
    stt = timed('episode_stats', v.episode_stats)
    assert all((x == 0).all() for x in stt.values())                  # (steps through the loop accumulate nothing; only rollouts do)
    offs = v.pack_layout()
    payload = torch.zeros(offs[7], dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    timed('pack_obs', lambda: v.pack_obs(payload.data_ptr()))
    want = (o.st.map[0].copy(), o.st.loc[0].copy(), int(o.st.facing[0]), o.st.inv[0].copy(), int(o.reward[0]), int(o.done[0]), int(o.info[0]))
    dst = [torch.zeros(n, dtype=torch.uint8, device='cuda') for n in (S * S, 8, 4, 4 * K, 4, 1, 4)]
    torch.cuda.synchronize()
    timed('unpack_obs', lambda: v.unpack_obs(payload.data_ptr(), 1, [x.data_ptr() for x in dst]))
    v.sync()
    h = [x.cpu().numpy() for x in dst]
    assert (h[0].view(np.int8) == want[0]).all() and (h[1].view(np.int32) == want[1]).all() and h[2].view(np.int32)[0] == want[2]
    assert (h[3].view(np.int32) == want[3]).all() and (h[4].view(np.int32)[0], h[5][0], h[6].view(np.uint32)[0]) == want[4:]
    s = torch.cuda.Stream()
    timed('stream_order', lambda: v.stream_order(s.cuda_stream, False))
    with torch.cuda.stream(s):
        m = v.device_observation()['map'].clone()
    s.synchronize()
    assert (m.cpu().numpy().reshape(-1) == o.st.map[0]).all()
    timed('timing_begin', v.timing_begin)
    timed('timing_mark', v.timing_mark)
    assert timed('timing_end', v.timing_end) >= 0
    timed('set_stream', lambda: v.set_stream(0))                       # (a fresh stream of the handle's own)
    timed('set_terminal_capture', lambda: v.set_terminal_capture(True))
    v.terminal_observation()                                           # (capture on: steps take a launch each; no loop to meet)
    v.set_terminal_capture(False)
    timed('lidar_configure fused', lambda: v.lidar_configure(lc, fused=True, dtype='packed'))
    state_ok('end')
    assert v.error_flags() == 0
    t0 = time.perf_counter()
    v.close()
    assert time.perf_counter() - t0 < LIMIT
