"""Rollouts and playouts behind their one request (csrc/ngw_abi_snapshot.cpp step_pairs, snapshot.pairs_call): which refusal wins when two arguments
are wrong at once - every text below was recorded from the build before the request existed -, and which C entry point each Python keyword
combination reaches (playout.pairs_symbol)."""
import ctypes as C

import numpy as np
import pytest

import ngw_testlib as T
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.playout import pairs_symbol
from gym_novel_gridworlds_amd.spec import make_spec

pytestmark = pytest.mark.gpu

N = None
BAD_FIELDS = 0x40                               # (a bit above NGW_KEY_ALL)
FIELDS_TEXT = "key fields 0x40: a non-empty selection of NGW_KEY_* bits expected"
NOT_OPEN = "not an open snapshot of this handle"


def _rollout(L, form, h, src, si, actions, stride, steps, dst, di, count, rep, limits=N, fields=0, keys=N, kstride=0, rew=N, rstride=0, obs=N, ostride=0):
    if form == 'plain':
        return L.ngw_snapshot_rollout(h, src, si, actions, stride, steps, dst, di, count, *rep)
    if form == 'path':
        return L.ngw_snapshot_rollout_path(h, src, si, actions, stride, steps, limits, dst, di, count, *rep, fields, keys, kstride)
    return L.ngw_snapshot_rollout_traj(h, src, si, actions, stride, steps, limits, dst, di, count, *rep, fields, keys, kstride, rew, rstride, obs, ostride)


def _playout(L, form, h, src, si, count, steps, dst, di, rep, rec=N, stride=0, limits=N, fields=0, keys=N, kstride=0, rew=N, rstride=0, obs=N, ostride=0):
    if form == 'plain':
        return L.ngw_snapshot_playout(h, src, si, count, steps, 1, 0, dst, di, *rep, N, rec, stride)
    if form == 'path':
        return L.ngw_snapshot_playout_path(h, src, si, count, steps, 1, 0, N, limits, dst, di, *rep, N, rec, stride, fields, keys, kstride)
    return L.ngw_snapshot_playout_traj(h, src, si, count, steps, 1, 0, N, limits, dst, di, *rep, N, rec, stride, fields, keys, kstride, rew, rstride, N, 0, obs,
                                       ostride)


def test_refusal_precedence_is_the_entry_points_own():
    """Two wrong arguments at once, through ctypes: the message is the one the entry point has always answered with, and nothing is touched."""
    import torch
    L, E, err = _cabi.lib(), _cabi.E_INVALID_ARG, _cabi.last_error
    spec = make_spec(T.POGO, 10)
    v = VecNovelGridworld(spec=spec, num_envs=64, seed=11)
    w = VecNovelGridworld(spec=spec, num_envs=64, seed=11)
    v.reset(); w.reset()
    s, foreign = v.snapshot(8), w.snapshot(8)
    before = v.get_state()
    buf = torch.zeros(4 * 64 * 16, dtype=torch.int64, device='cuda')          # (one 16-byte aligned buffer stands in for every device argument)
    torch.cuda.synchronize()
    p = C.c_void_p(buf.data_ptr())
    rep, none = (p, N, N, N), (N, N, N, N)
    h = v._h
    for kind, call in (('rollout', lambda form, *a, **k: _rollout(L, form, h, *a, **k)), ('playout', lambda form, *a, **k: _playout(L, form, h, *a, **k))):
        R = kind == 'rollout'
        # a reward stride below count and destination slots without a destination (traj): the stride text wins
        rc = call('traj', N, N, p, 8, 3, N, p, 8, rep, rew=p, rstride=7) if R else call('traj', N, N, 8, 3, N, p, rep, rew=p, rstride=7)
        assert rc == E and err() == "%s of 8 pairs with a reward stride of 7" % kind
        # bad key fields and count above the destination's capacity (path): the capacity text wins
        rc = call('path', N, N, p, 9, 3, s._s, N, 9, rep, fields=BAD_FIELDS, keys=p, kstride=9) if R else \
            call('path', N, N, 9, 3, s._s, N, rep, fields=BAD_FIELDS, keys=p, kstride=9)
        assert rc == E and err() == "%s of 9 states into a snapshot of 8 slots" % kind
        # ... while the trajectory form checks its own arguments first: the fields text wins there
        rc = call('traj', N, N, p, 9, 3, s._s, N, 9, rep, fields=BAD_FIELDS, keys=p, kstride=9) if R else \
            call('traj', N, N, 9, 3, s._s, N, rep, fields=BAD_FIELDS, keys=p, kstride=9)
        assert rc == E and err() == FIELDS_TEXT
        # observations before ngw_lidar_configure and bad key fields (traj): the fields text wins
        rc = call('traj', N, N, p, 8, 3, N, N, 8, rep, fields=BAD_FIELDS, keys=p, kstride=8, obs=p, ostride=64) if R else \
            call('traj', N, N, 8, 3, N, N, rep, fields=BAD_FIELDS, keys=p, kstride=8, obs=p, ostride=64)
        assert rc == E and err() == FIELDS_TEXT
        rc = call('traj', N, N, p, 8, 3, N, N, 8, rep, obs=p, ostride=64) if R else call('traj', N, N, 8, 3, N, N, rep, obs=p, ostride=64)
        assert rc == E and err() == "ngw_snapshot_%s_traj with observations before ngw_lidar_configure" % kind
        for form in ('plain', 'path', 'traj'):
            # n_steps = 0 and NULL actions (rollout): "NULL argument" wins; a playout needs no actions: its steps text, ahead of a negative count
            rc = call(form, N, N, N, 8, 0, N, N, 8, rep) if R else call(form, N, N, -1, 0, N, N, rep)
            assert rc == E and err() == ("NULL argument" if R else "playout of 0 steps")
            # a key (or plan / action) stride below count and a snapshot of another handle: the stride text wins
            rc = call(form, foreign._s, N, p, 7, 3, N, N, 8, rep) if R else call(form, foreign._s, N, 8, 3, N, N, rep, rec=p, stride=7)
            assert rc == E and err() == ("rollout of 8 pairs with a pair stride of 7" if R else "playout of 8 pairs with an action stride of 7")
            # a snapshot of another handle and more pairs than envs: "not an open snapshot" wins (source and destination alike)
            rc = call(form, foreign._s, N, p, 65, 3, N, N, 65, rep) if R else call(form, foreign._s, N, 65, 3, N, N, rep)
            assert rc == E and err() == NOT_OPEN
            rc = call(form, N, N, p, 65, 3, foreign._s, N, 65, rep) if R else call(form, N, N, 65, 3, foreign._s, N, rep)
            assert rc == E and err() == NOT_OPEN
            # destination slots without a destination and a snapshot of another handle: the slots text wins
            rc = call(form, foreign._s, N, p, 8, 3, N, p, 8, rep) if R else call(form, foreign._s, N, 8, 3, N, p, rep)
            assert rc == E and err() == "destination slots without a destination snapshot"
            # more pairs than envs without a list
            rc = call(form, N, N, p, 65, 3, N, N, 65, rep) if R else call(form, N, N, 65, 3, N, N, rep)
            assert rc == E and err() == "%s of 65 states from 64 envs" % kind
            rc = call(form, s._s, N, p, 9, 3, N, N, 9, rep) if R else call(form, s._s, N, 9, 3, N, N, rep)
            assert rc == E and err() == "%s of 9 states from 8 slots" % kind
            if R:                               # no destination and no report, from a snapshot of another handle: "nothing to do" wins
                assert call(form, foreign._s, N, p, 8, 3, N, N, 8, none) == E and err() == "rollout without a destination and without a report: nothing to do"
            else:                               # (a playout's every output may be NULL: the foreign snapshot is what is wrong)
                assert call(form, foreign._s, N, 8, 3, N, N, none) == E and err() == NOT_OPEN
    v.sync()
    after = v.get_state()
    assert v.error_flags() == 0 and all((before[k] == after[k]).all() for k in before)
    assert (buf == 0).all()                     # no refused call launched anything
    v.close(); w.close()


def test_map_limits_per_form():
    """The form is the entry point's: where the handle's own layout is beyond 160 KiB (Pogostick 48 x 48; 47 x 47 still fits) every one of the six
    answers the plain refusal under its own name.  (The path form's own limit: test_path_limit_where_it_binds_alone.)"""
    import torch
    L, E, err = _cabi.lib(), _cabi.E_INVALID_ARG, _cabi.last_error
    plans, ret = torch.zeros(3 * 64, dtype=torch.int32, device='cuda'), torch.zeros(64, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    p, rep = C.c_void_p(plans.data_ptr()), (C.c_void_p(ret.data_ptr()), N, N, N)
    for S, refused in ((47, False), (48, True)):
        v = VecNovelGridworld(spec=make_spec(T.POGO, S), num_envs=64, seed=5)
        v.reset()
        for form, suffix in (('plain', ''), ('path', '_path'), ('traj', '_traj')):
            for kind in ('rollout', 'playout'):
                rc = _rollout(L, form, v._h, N, N, p, 64, 3, N, N, 64, rep) if kind == 'rollout' else _playout(L, form, v._h, N, N, 64, 3, N, N, rep)
                if refused:
                    assert rc == E and err() == ("map_size 48: this call keeps a wavefront's 64 maps in LDS (ngw_snapshot_%s%s, as the fused rollouts) and they need "
                                                 "more than 160 KiB; per-launch steps and resets are available" % (kind, suffix))
                else:
                    assert rc == 0, (S, form, kind, err())
        v.sync()
        assert v.error_flags() == 0
        v.close()


def _lds_bytes_of(make):
    """make() -> an env, with the library's "[ngw] LDS per wavefront: N B" lines (NGW_DEBUG_LDS) read off stderr -> (env, the last N: the layout in force)."""
    import os, re, tempfile
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            env = make()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        found = re.findall(r'LDS per wavefront: (\d+) B \(S = ', f.read().decode())
    return env, int(found[-1])


def test_path_limit_where_it_binds_alone(monkeypatch):
    """The smallest map at which NGW_PATH_LDS_BYTES (the handle's LDS bytes + 64 * 4 * KP of inventory shadows) is beyond 160 KiB while the handle's own
    layout still fits - found from the bytes the library reports, not guessed; with the fused int32 lidar row of 8 beams that is Pogostick 45 x 45
    (162 128 + 2 304 B).  There the plain calls run, the path calls answer the path refusal AFTER the checks all forms share, and the trajectory calls
    answer it AHEAD of them."""
    import torch
    monkeypatch.setenv('NGW_DEBUG_LDS', '1')
    L, E, err, MAX = _cabi.lib(), _cabi.E_INVALID_ARG, _cabi.last_error, 160 * 1024

    def make(S):
        e = VecNovelGridworld(spec=make_spec(T.POGO, S), num_envs=64, seed=5)
        e.lidar_configure(num_beams=8, fused=True, dtype=np.int32)
        return e
    v = None
    for S in range(40, 48):
        v, lds = _lds_bytes_of(lambda: make(S))
        KP = v.n_items | 1
        need = lds + 64 * 4 * KP
        if lds <= MAX < need:
            break
        assert need <= MAX, "map_size %d: %d B, the handle's own layout is beyond the limit before the path form's is" % (S, lds)
        v.close()
    assert S == 45 and need == 164432
    v.reset()
    plans, ret = torch.zeros(3 * 65, dtype=torch.int32, device='cuda'), torch.zeros(65, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    p, rep = C.c_void_p(plans.data_ptr()), (C.c_void_p(ret.data_ptr()), N, N, N)
    text = ("map_size %d: this call keeps a wavefront's 64 maps and a second copy of their inventories in LDS (ngw_snapshot_%%s_%%s) and they need %d B, "
            "more than 160 KiB; the plain call is available" % (S, need))
    for kind in ('rollout', 'playout'):
        call = (lambda form, n: _rollout(L, form, v._h, N, N, p, 65, 3, N, N, n, rep)) if kind == 'rollout' else \
            (lambda form, n: _playout(L, form, v._h, N, N, n, 3, N, N, rep))
        assert call('plain', 64) == 0, err()
        assert call('path', 64) == E and err() == text % (kind, 'path')
        assert call('traj', 64) == E and err() == text % (kind, 'traj')
        # with more pairs than envs too: the path form's limit comes after that check, the trajectory form's ahead of it
        assert call('path', 65) == E and err() == "%s of 65 states from 64 envs" % kind
        assert call('traj', 65) == E and err() == text % (kind, 'traj')
    v.sync()
    assert v.error_flags() == 0
    v.close()


class _Recorder:
    """_cabi.lib() with every call of a rollout / playout entry point noted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(('ngw_snapshot_rollout', 'ngw_snapshot_playout')):
            return fn

        def noted(*args):
            self.calls.append(name)
            return fn(*args)
        return noted


# the keyword sets and the entry point each reaches from Snapshot.rollout / Snapshot.playout and env.playouts (None: the call has no such keyword)
ROUTES = [
    ({}, 'ngw_snapshot_rollout', 'ngw_snapshot_playout'),
    ({'limits': [3, 2, 1, 0]}, 'ngw_snapshot_rollout_path', 'ngw_snapshot_playout_path'),
    ({'path_keys': True}, 'ngw_snapshot_rollout_path', 'ngw_snapshot_playout_path'),
    ({'weights': 'w'}, None, 'ngw_snapshot_playout_weighted'),
    ({'rewards': True}, 'ngw_snapshot_rollout_traj', 'ngw_snapshot_playout_traj'),
    ({'masks': True}, None, 'ngw_snapshot_playout_traj'),
    ({'observe': 'lidar'}, 'ngw_snapshot_rollout_traj', 'ngw_snapshot_playout_traj'),
    ({'weights': 'w', 'path_keys': True}, None, 'ngw_snapshot_playout_path'),
]


def test_every_keyword_set_makes_one_call_to_its_entry_point(monkeypatch):
    spec = make_spec(T.POGO, 10)
    v = VecNovelGridworld(spec=spec, num_envs=64, seed=2)
    small = VecNovelGridworld(spec=spec, num_envs=4, seed=2)                  # (playouts: 4 envs x 1 playout are the 4 pairs)
    for e in (v, small):
        e.reset()
        e.lidar_configure(num_beams=8)
    s = v.snapshot(8)
    s.save(envs=np.arange(8), slots=np.arange(8))
    rec = _Recorder(_cabi.lib())
    monkeypatch.setattr(_cabi, 'lib', lambda: rec)
    parents, plans = np.arange(4), np.zeros((4, 3), np.int64)
    weights = np.ones(v.n_actions, np.float32)
    for kw, rollout, playout in ROUTES:
        kw = {k: (weights if x == 'w' else x) for k, x in kw.items()}
        path, traj = 'limits' in kw or 'path_keys' in kw, bool({'rewards', 'masks', 'observe'} & set(kw))
        assert playout == pairs_symbol('playout', 'weights' in kw, path, traj) and rollout in (None, pairs_symbol('rollout', False, path, traj))
        if rollout:
            rec.calls.clear()
            r = s.rollout(parents, plans, **kw)
            assert rec.calls == [rollout] and r.length.shape == (4,)
        rec.calls.clear()
        r = s.playout(parents, 3, 7, **kw)
        assert rec.calls == [playout] and r.length.shape == (4,)
        if 'limits' not in kw:
            rec.calls.clear()
            r = small.playouts(1, 3, 7, **kw)
            assert rec.calls == [playout] and r.length.shape == (4, 1)
    assert v.error_flags() == 0 and small.error_flags() == 0
    monkeypatch.undo()
    v.close(); small.close()
