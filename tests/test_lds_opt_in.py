"""The opt-in to more than 64 KiB of dynamic LDS, made by every launcher in a FRESH process (csrc/ngw_launch.inc).

The opt-in is remembered per process, kernel and device.  In the rest of the suite a kernel may already have been opted in by an earlier,
larger handle of the same process, so a launcher that forgot the opt-in would still pass there.  A missing opt-in is not a fault: the launch
returns a HIP error and the entry point NGW_E_HIP, which the Python layer raises.  So this test starts ONE child process and lets it meet every
launcher that can ask for more than 64 KiB for the first time, on the smallest maps that do: a wavefront's staged maps take 64 * S * S bytes,
more than 64 KiB from S = 33 on, and the three map addressing modes (ngw_abi_create.cpp: S odd -> byte, S = 2 mod 4 -> straight,
S = 0 mod 4 -> dword) first reach that at

    S = 33 (byte), S = 34 (straight), S = 36 (dword);      S = 35 (byte again, in the same process: the request GREW)

Per size, on a 64-env handle (one wavefront), everything held to the CPU oracle as the neighbouring tests do: explicit resets through the
general kernel (NGW_FAST_RESET=0 in the child's environment; with and without the fused lidar), the stand-alone lidar launch, a step through
the staged kernel with the fused marched lidar, fused rollouts with generated and with supplied actions, ngw_plan_eval with 2 plans x 3 steps.
Then the bit-row rebuild behind ngw_set_state with a map at 32 x 32 with the default 8 beams (64 padded dword-mode maps + the word tile:
72.5 KiB), and a one-env adapter at 33 x 33 whose step() calls launch the resident loop kernel (64 padded maps: 69 KiB)."""
import os
import subprocess
import sys

import pytest

SIZES = (33, 35, 34, 36)            # byte, byte (larger: the request grew), straight, dword
BOARDS_SIZE = 32                    # the largest map with occupancy bit rows
SOLO_SIZE = 33


@pytest.mark.gpu
def test_every_launcher_opts_in_above_64_kib_in_a_fresh_process():
    env = dict(os.environ, NGW_FAST_RESET='0')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, "the child failed:\n%s\n%s" % (out.stdout[-3000:], out.stderr[-3000:])
    for S in SIZES:
        assert 'staged kernels S=%d ok' % S in out.stdout, out.stdout
    assert 'bit-row rebuild ok' in out.stdout and 'one-env loop ok' in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------------------------- the child process
def _state_equal(v, o, where):
    import numpy as np
    hs, st = v.get_state(), o.st
    for k, want in (('map', st.map), ('loc', st.loc), ('facing', st.facing), ('inv', st.inv), ('selected', st.selected),
                    ('step_count', st.step_count), ('episode', st.episode)):
        bad = np.nonzero((hs[k] != want).reshape(len(hs[k]), -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs for %d envs, first env %d" % (where, k, bad.size, bad[0])


def _outs_equal(v, o, where):
    reward, done, info = v.get_step_out(copy=True)
    assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), where
    assert (info['result'] == o.result.astype(bool)).all() and (info['step_cost_code'] == o.cost_code).all(), where
    assert (info['message_code'] == o.msg_code).all() and (info['message_arg'] == o.msg_arg).all(), where


def _lidar_equal(v, o, cc, spec, where):
    from oracle.ngw_oracle import lidar
    got = v.lidar_observation()
    exp = lidar(cc, spec.map_size, len(spec.items_id), o.st.map, o.st.loc, o.st.facing, o.st.inv)
    assert (got == exp).all(), where


def _staged_kernels(S):
    import numpy as np
    import torch
    import ngw_testlib as T
    import plan_oracle as PO
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    from gym_novel_gridworlds_amd.spec import make_spec
    from oracle.ngw_oracle import Oracle
    spec = make_spec(T.POGO, S)
    n, A, H = 64, len(spec.actions_id), 9
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=S, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=S, autoreset=True, horizon=H)
    rs = np.random.RandomState(S)
    w = 'S=%d ' % S
    v.reset(); assert o.reset() == 0                                   # the general kernel (NGW_FAST_RESET=0)
    _state_equal(v, o, w + 'reset')
    v.rollout(H + 3, action_seed=7, t0=2); assert o.rollout(H + 3, 7, 2) == 0      # generated actions, across an episode end
    _state_equal(v, o, w + 'rollout'); _outs_equal(v, o, w + 'rollout')
    acts = torch.from_numpy(rs.randint(0, A, (H + 2, n)).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    v.rollout_actions(acts.data_ptr(), n, H + 2)                       # supplied actions
    for row in acts.cpu().numpy():
        assert o.step(np.ascontiguousarray(row)) == 0
    _state_equal(v, o, w + 'rollout_actions'); _outs_equal(v, o, w + 'rollout_actions')
    plans = rs.randint(0, A, (n, 2, 3))                                # ngw_plan_eval: 2 plans x 3 steps
    PO.assert_plans(v.evaluate_plans(plans, copy=True), PO.oracle_plans(spec, o.st, plans, autoreset=True, horizon=H), w + 'plans')
    lc = LidarConfig(spec, 8)
    cc = lc.compile(spec)
    v.lidar_configure(lc, fused=False, dtype=np.int32)                 # the stand-alone lidar launch
    _lidar_equal(v, o, cc, spec, w + 'stand-alone lidar')
    v.lidar_configure(lc, fused=True, dtype=np.int32)                  # fused: no bit rows beyond 32 x 32, so the staged kernels march
    assert not v.step_reads_map_in_place
    v.reset(); assert o.reset() == 0                                   # the general kernel with the fused lidar epilogue
    _state_equal(v, o, w + 'reset, fused lidar'); _lidar_equal(v, o, cc, spec, w + 'reset, fused lidar')
    a = rs.randint(0, A, n).astype(np.int32)
    v.step(a); assert o.step(a) == 0                                   # the staged step kernel with the fused marched lidar
    _state_equal(v, o, w + 'step, fused lidar'); _outs_equal(v, o, w + 'step, fused lidar'); _lidar_equal(v, o, cc, spec, w + 'step, fused lidar')
    assert v.error_flags() == 0
    v.close()
    print('staged kernels S=%d ok' % S, flush=True)


def _bit_row_rebuild():
    import numpy as np
    import ngw_testlib as T
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    from gym_novel_gridworlds_amd.spec import make_spec
    from oracle.ngw_oracle import Oracle
    S = BOARDS_SIZE
    spec = make_spec(T.POGO, S)
    n = 64
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=3)
    o = Oracle(spec.compile(), n, seed=3)
    lc = LidarConfig(spec, 8)                                          # the default 8 beams: the observation comes from the bit rows
    cc = lc.compile(spec)
    v.lidar_configure(lc, fused=True, dtype=np.int32)
    v.reset(); assert o.reset() == 0
    m = o.st.map.reshape(n, S, S).copy()                               # a block next to every agent that has air there: the rays must see it
    for e in range(n):
        r, c = o.st.loc[e]
        if c + 1 < S - 1 and m[e, r, c + 1] == 0:
            m[e, r, c + 1] = spec.items_id['tree_log']
    v.set_state(0, map=m.reshape(n, -1)); o.st.map[:] = m.reshape(n, -1)   # maps rewritten behind the kernels' back: the next step rebuilds the bit rows
    a = np.full(n, spec.actions_id['Left'], np.int32)
    for t in range(2):
        v.step(a); assert o.step(a) == 0
        _state_equal(v, o, 'bit rows, turn %d' % t); _lidar_equal(v, o, cc, spec, 'bit rows, turn %d' % t)
    assert v.error_flags() == 0
    v.close()
    print('bit-row rebuild ok', flush=True)


def _one_env_loop():
    import ctypes as C
    import numpy as np
    import gym_novel_gridworlds_amd as G
    import ngw_testlib as T
    from gym_novel_gridworlds_amd import _cabi

    def adapter(backend):
        env = G.make(T.POGO)
        if backend == 'oracle':
            env._make_backend = lambda spec, seed_: T.OracleVec(spec, 1, seed=seed_)
        env.seed(5)
        env.map_size = SOLO_SIZE
        return env

    def same(x, y):
        if isinstance(x, tuple):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, np.ndarray):
            return x.shape == np.shape(y) and (x == y).all()
        return x == y

    hip, twin = adapter('hip'), adapter('oracle')
    assert same(hip.reset(), twin.reset()), 'one-env reset'
    rs = np.random.RandomState(1)
    for t in range(8):
        a = int(rs.randint(0, len(hip.actions_id)))
        assert same(hip.step(a), twin.step(a)), ('one-env step', t, a)
    starts = _cabi.lib().ngw_debug_solo_starts
    starts.argtypes, starts.restype = [C.c_void_p], C.c_longlong
    assert os.environ.get('NGW_SOLO') == '0' or sum(int(starts(v._h)) for v in hip._vec_cache.values()) >= 1, 'the resident loop never started'
    hip.close()
    print('one-env loop ok', flush=True)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ngw_oracle
    ngw_oracle.build()
    for size in SIZES:
        _staged_kernels(size)
    _bit_row_rebuild()
    _one_env_loop()
