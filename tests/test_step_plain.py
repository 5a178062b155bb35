"""The in-place step kernel's instantiation for the plain spec class (ngw_step_lean<..., PLAIN>): parity with the oracle where it runs,
the general instantiation - and the same parity - on every boundary of the class, the NGW_STEP_PLAIN=0 switch, and the class predicate's
4 GB bound (asked with made-up spans, on the CPU).  Run as a script this file is the child process of the switch test."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = (('map', 'map'), ('loc', 'loc'), ('facing', 'facing'), ('inv', 'inv'), ('selected', 'selected'), ('step_count', 'step_count'), ('episode', 'episode'))


def _compare(v, o, flags_want, where, digest=None):
    """map, inventory, pose, facing, selected, step_count (and the episode counters), reward, done, info, error flags against the oracle"""
    hs = v.get_state()
    for k, ok in STATE:
        want = getattr(o.st, ok)
        bad = np.nonzero((hs[k] != want).reshape(len(hs[k]), -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs for %d envs, first env %d" % (where, k, bad.size, bad[0])
    out = {k: t.cpu().numpy() for k, t in v.device_outputs().items()}
    assert (out['reward'] == o.reward).all(), where + ': reward'
    assert (out['done'] == o.done).all(), where + ': done'
    assert (out['info'].view(np.uint32) == o.info.view(np.uint32)).all(), where + ': info'
    flags = v.error_flags()
    assert flags == flags_want, '%s: error flags %d, oracle %d' % (where, flags, flags_want)
    if digest is not None:
        for k, _ in STATE:
            digest.update(np.ascontiguousarray(hs[k]).tobytes())
        for k in ('reward', 'done', 'info'):
            digest.update(np.ascontiguousarray(out[k]).tobytes())
        digest.update(bytes([flags & 255]))


def _actions(A, n, steps, seed, bad_row):
    a = np.random.RandomState(seed).randint(0, A, size=(steps, n)).astype(np.int32)
    if bad_row is not None:                                             # one row of out-of-range ids: the envs stay as they are, the flag goes up
        a[bad_row] = A + np.arange(n) % 3
        a[bad_row, ::7] = -1
    return a


def plain_scenario(want_plain):
    """Pogostick-v1 10 x 10, 130 envs (two full waves and a 2-lane tail), autoreset with horizon 7 (cold path: prepared rows while the refill
    keeps up, stale ones after), 60 eager steps - one row of them invalid - then a 16-step graph replayed four times.  Returns a digest."""
    import torch
    import ngw_testlib as T
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from oracle.ngw_oracle import Oracle
    n, H = 130, 7
    spec = T.build_spec('pogo10')
    A = len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=3, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=3, autoreset=True, horizon=H)
    v.reset(); o.reset()
    assert v.step_reads_map_in_place and v.step_kernel_plain[0] == want_plain
    d = hashlib.sha256()
    acts = _actions(A, n, 60, 11, 23)
    dev = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()
    for t in range(60):
        v.step_device(dev[t].data_ptr())
        want = o.step(acts[t])
        assert v.step_kernel_plain[1] == want_plain
        _compare(v, o, want, 'eager step %d' % t, d)
    assert o.st.episode.min() >= 8                                      # (the cold path ran, many times per env)
    g = _actions(A, n, 16, 12, 5)
    gdev = torch.from_numpy(g).cuda()
    torch.cuda.synchronize()
    v.graph_build(gdev.data_ptr(), n, 16)
    for rep in range(4):
        v.graph_launch(1)
        want = 0
        for t in range(16):
            want |= o.step(g[t])
        _compare(v, o, want, 'graph replay %d' % rep, d)
    assert v.step_kernel_plain == (want_plain, want_plain)
    v.close()
    return d.hexdigest()


_digest = {}
# (the suite also runs under NGW_STEP_PLAIN=0: the same parity then, from the general instantiation - the library reads the switch with atoi)
_PLAIN_ON = os.environ.get('NGW_STEP_PLAIN', '1').strip().lstrip('+').lstrip('0')[:1].isdigit() or 'NGW_STEP_PLAIN' not in os.environ


def _plain_digest():
    if 'plain' not in _digest:
        _digest['plain'] = plain_scenario(_PLAIN_ON)
    return _digest['plain']


@pytest.mark.gpu
def test_plain_class_matches_oracle_eager_and_graph():
    assert len(_plain_digest()) == 64


ADD4 = (('additem', 'easy', 'arrow', ''), ('additem', 'medium', 'gold', ''), ('additem', 'hard', 'paper', ''), ('additem', 'easy', 'spring', ''))


def _spec(cfg):
    import ngw_testlib as T
    if cfg != 'add4_12':
        return T.build_spec(cfg)
    from gym_novel_gridworlds_amd.novelty import apply_novelty
    from gym_novel_gridworlds_amd.spec import make_spec
    spec = make_spec(T.POGO, 12)                                        # four AddItem novelties on a 12 x 12 map: 13 items
    for nov in ADD4:
        apply_novelty(spec, *nov)
    return spec


def _boundary(cfg, n=130, steps=30, horizon=9, setup=None, host=False):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld
    from oracle.ngw_oracle import Oracle
    spec = _spec(cfg)
    A = len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=5, autoreset=True, horizon=horizon)
    o = Oracle(spec.compile(), n, seed=5, autoreset=True, horizon=horizon)
    v.reset(); o.reset()
    if setup:
        setup(v)
    acts = _actions(A, n, steps, 13, None if host else 4)
    dev = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()
    for t in range(steps):
        if host:
            _, reward, done, info = v.step(acts[t])
            assert o.step(acts[t]) == 0
            assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        else:
            v.step_device(dev[t].data_ptr())
            want = o.step(acts[t])
        assert v.step_kernel_plain[1] is False, '%s: the general instantiation runs here (step %d)' % (cfg, t)
        _compare(v, o, 0 if host else want, '%s step %d' % (cfg, t))
    v.close()
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', ['jump12', 'add4_12', 'axe10', 'fire10h'])
def test_outside_the_class_the_general_kernel_runs(cfg):
    """a Jump action; more than 12 items (four AddItem novelties at 12 x 12); the axe novelty, which brings an entity; a FireWall spec (wrapper predicates)"""
    spec = _boundary(cfg)
    if cfg == 'add4_12':
        assert len(spec.items_id) > 12
    if cfg == 'axe10':
        assert spec.compile().n_entities > 0


@pytest.mark.gpu
def test_fused_lidar_takes_the_general_kernel():
    _boundary('pogo10', setup=lambda v: v.lidar_configure(fused=True))


@pytest.mark.gpu
def test_action_masks_take_the_general_kernel():
    _boundary('pogo10', setup=lambda v: v.set_action_masks(True))


@pytest.mark.gpu
def test_host_api_on_one_wavefront_takes_the_general_kernel():
    _boundary('pogo10', n=64, host=True)


@pytest.mark.gpu
def test_switch_forces_the_general_kernel_with_identical_outputs():
    env = dict(os.environ, NGW_STEP_PLAIN='0')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, "the child failed:\n%s\n%s" % (out.stdout[-3000:], out.stderr[-3000:])
    assert 'general digest ' + _plain_digest() in out.stdout, out.stdout[-2000:]


def test_class_predicate_refuses_what_32_bits_cannot_address():
    from gym_novel_gridworlds_amd import _cabi
    f = _cabi.lib().ngwh_step_plain_class
    f.argtypes, f.restype = [C.c_int32] * 5 + [C.c_uint64] * 2, C.c_int
    ok = (9, 0, 0, 5, 5, 65536 * 353, 65536 * 4)                        # Pogostick-v1 at 65 536 envs
    assert f(*ok) == 1
    assert f(9, 0, 0, 5, 5, 2 ** 32, 65536 * 4) == 0                     # a slab that spans 2^32 bytes
    assert f(9, 0, 0, 5, 5, 2 ** 32 - 1, 2 ** 32 - 1) == 1
    assert f(9, 0, 0, 5, 5, 65536 * 353, 2 ** 32) == 0                   # ... an output array that does
    assert f(13, 0, 0, 5, 5, 1000, 1000) == 0 and f(12, 0, 0, 5, 5, 1000, 1000) == 1
    assert f(9, 1, 0, 5, 5, 1000, 1000) == 0                             # a Jump action
    assert f(9, 0, 1, 5, 5, 1000, 1000) == 0                             # entities
    assert f(9, 0, 0, 5, 6, 1000, 1000) == 0                             # two "near" items


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    print('general digest ' + plain_scenario(False))
