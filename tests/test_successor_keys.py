"""Successor keys on the MI355X (csrc/ngw_successors.inc, include/ngw.h ngw_successor_keys, Snapshot.successor_keys / insert_successor_keys,
VecNovelGridworld.successor_keys, the adapter's and the wrappers' forwards), held to the two CPU oracles: the expected children are
expand_oracle.oracle_expand's on a host copy of the parent rows, their keys state_key_oracle.keys_of's, the reports the same oracle_expand's
(tests/successor_key_oracle.py) - never the device's own expand or keys, except where a test says that it compares the two routes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expand_oracle as XO
import ngw_testlib as T
import state_key_oracle as SK
import successor_key_oracle as SKO
from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi
from gym_novel_gridworlds_amd.snapshot import SuccessorKeys, fresh_pairs
from gym_novel_gridworlds_amd.spec import F_BAD_INDEX, make_spec
from oracle.ngw_oracle import Oracle

pytestmark = pytest.mark.gpu
CFG_ALL = sorted(T.CFGS)
FIELDS = (SK.STATE, SK.ALL) + SK.SINGLE
LDS_MAX = 160 * 1024


def lds_bytes(S, K):
    """What the call keeps in LDS, computed the way the library does: two sets of 64 rows, a map MS bytes (an odd number of dwords, or S*S
    itself where that is one) and an inventory row of KP = K | 1 dwords each."""
    S2 = S * S
    dw = (S2 + 3) // 4
    MS = S2 if (S2 % 4 == 0 and dw % 2 == 1) else (dw if dw % 2 else dw + 1) * 4
    return 2 * 64 * (MS + 4 * (K | 1))


def dev_i32(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize('cfg', CFG_ALL)
def test_every_configuration(cfg):
    """130 envs (two full waves and a partial one), right after reset and after 60 random steps, autoreset off and on under a horizon of 25,
    from the envs and from slots through a repeated random index list, under KEY_STATE, KEY_ALL and every single bit: all 130 x A keys and
    reports equal the oracles'; for the envs the reports also equal the lookahead table entry for entry.  A configuration whose maps are
    beyond the call's limit is refused instead, by name."""
    spec = T.build_spec(cfg)
    n, A, K = 130, len(spec.actions_id), len(spec.items_id)
    seed = XO.good_seed(spec, n)
    rs = np.random.RandomState(13)
    for auto in (False, True):
        kw = dict(autoreset=True, horizon=25) if auto else {}
        v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, **kw)
        o = Oracle(spec.compile(), n, seed=seed, **kw)
        v.reset(); o.reset()
        pool = v.snapshot(n)
        if lds_bytes(spec.map_size, K) > LDS_MAX:
            with pytest.raises(_cabi.NgwError, match='map_size %d.*ngw_snapshot_expand followed by ngw_state_keys' % spec.map_size):
                v.successor_keys()
            with pytest.raises(_cabi.NgwError, match='two sets of a wavefront'):
                pool.successor_keys()
            v.close()
            continue
        for stage in ('after reset', 'after random play'):
            if stage == 'after random play':
                for t in range(60):
                    a = rs.randint(0, A, n).astype(np.int32)
                    if o.step(a) & 2:                           # a tight map exhausted the placement of an autoreset: stop here
                        break
                    v.step(a)
            where = '%s %s auto=%d' % (cfg, stage, auto)
            exp = SKO.Successors(spec, o.st, np.arange(n), v.autoreset, v.horizon)
            pool.save()
            slots = rs.randint(0, n, n)                         # slot i holds env i: the same parents, some of them several times
            exp_slots = SKO.Successors(spec, o.st, slots, v.autoreset, v.horizon)
            for fields in FIELDS:
                s = v.successor_keys(fields=fields)
                SKO.assert_successors(s, exp, fields, where + ' envs')
                SKO.assert_successors(pool.successor_keys(slots, fields), exp_slots, fields, where + ' slots')
            look = v.lookahead(copy=True)
            assert (s.reward == look.reward).all() and (s.done == look.done).all() and (s.info == look.info).all(), where
            assert (s.result == look.result).all(), where
        assert v.error_flags() == 0
        v.close()


@pytest.mark.parametrize('S', [9, 10, 12, 24, 32])
@pytest.mark.parametrize('count', [1, 63, 65, 200])
def test_map_sizes_and_counts(S, count):
    """One map size per staging form (odd S*S with a byte tail: 9, dwords: 10, 16-byte pieces: 12), a size whose two row sets need the LDS
    opt-in above 64 KiB (24) and 32; counts around the wavefront width and far above num_envs = 5, so parents repeat heavily; host
    lists from the envs, device tensors from slots with the results left on the device - and taken in place by the key table."""
    import torch
    spec = make_spec(T.POGO, S)
    n, A, K = 5, len(spec.actions_id), len(spec.items_id)
    assert (lds_bytes(S, K) > 64 * 1024) == (S >= 24)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=30)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=30)
    v.reset(); o.reset()
    rs = np.random.RandomState(S + count)
    for t in range(25):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    where = 'S=%d count=%d' % (S, count)
    envs = rs.randint(0, n, count)
    exp = SKO.Successors(spec, o.st, envs, True, 30)
    s = v.successor_keys(envs, SK.ALL)
    assert s.keys.dtype == np.uint64 and s.reward.dtype == np.int32 and s.done.dtype == np.bool_ and s.info.dtype == np.uint32
    SKO.assert_successors(s, exp, SK.ALL, where + ' host list')
    SKO.assert_successors(v.successor_keys(envs, SK.MAP | SK.INV, reports=False), exp, SK.MAP | SK.INV, where + ' no reports', reports=False)
    pool = v.snapshot(n)
    pool.save()
    d = pool.successor_keys(dev_i32(envs), SK.STATE, device=True)
    assert isinstance(d, SuccessorKeys) and all(isinstance(x, torch.Tensor) and tuple(x.shape) == (count, A) for x in d)
    assert (d.keys.dtype, d.reward.dtype, d.done.dtype, d.result.dtype, d.info.dtype) == (torch.int64, torch.int32, torch.bool, torch.bool, torch.int32)
    SKO.assert_successors(d, exp, SK.STATE, where + ' device tensors')
    assert (d.goal.cpu().numpy() == (exp.rep['done'] & ((exp.rep['info'] >> 1) & 1).astype(bool))).all()
    table = v.key_table(count * A)
    flat = d.keys.reshape(-1)
    assert flat.data_ptr() == d.keys.data_ptr() and flat.is_contiguous()
    found = table.insert(flat)                                   # the flattened tensor in place
    keys = exp.keys(SK.STATE).reshape(-1)
    assert found.fresh.sum() == len(set(keys.tolist())) == len(table)
    first = np.zeros(count * A, bool)
    first[np.unique(keys, return_index=True)[1]] = True
    assert (found.fresh == first).all()
    assert v.error_flags() == 0
    v.close()


@pytest.mark.parametrize('cfg', ['axe10', 'fire10h'])
def test_the_route_it_replaces_gives_the_same_bits(cfg):
    """expand_all into a scratch pool followed by keys of the children equals successor_keys bit for bit, and the Expansion equals the
    reports: a configuration with pick-ups in the 3 x 3 window and one with FireWall deaths, after play, under autoreset and a horizon."""
    spec = T.build_spec(cfg)
    n, A = 130, len(spec.actions_id)
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=20)
    v.reset()
    rs = np.random.RandomState(3)
    scratch = v.snapshot(n * A)
    for stage in range(3):
        for t in range(13):
            v.step(rs.randint(0, A, n).astype(np.int32))
        e = scratch.expand_all(np.arange(n), 0, from_envs=True)
        for fields in (SK.STATE, SK.ALL):
            s = v.successor_keys(fields=fields)
            assert (s.keys.reshape(-1) == scratch.keys(fields=fields)).all(), (cfg, stage, fields)
            assert all((s[k] == e[k]).all() for k in ('reward', 'done', 'result', 'info')), (cfg, stage)
    assert v.error_flags() == 0
    v.close()


def _everything(v, snaps):
    st = v.get_state()
    reward, done, info = v.get_step_out(copy=True)
    out = {k: st[k].copy() for k in XO.STATE_KEYS}
    out.update(reward=reward, done=done, words=v.action_mask_words(copy=True))
    out.update({'info_' + k: np.asarray(info[k]).copy() for k in ('result', 'step_cost_code', 'message_code', 'message_arg')})
    out.update({'look_' + k: np.asarray(x) for k, x in zip(('reward', 'done', 'result', 'info'), v.lookahead(copy=True))})
    for i, s in enumerate(snaps):
        out.update({'snap%d_%s' % (i, k): x for k, x in s.state().items()})
    return out


@pytest.mark.parametrize('cfg', ['pogo10', 'fire10h'])
def test_nothing_is_committed(cfg):
    """Calls of every kind leave the state, the last step's outputs, the mask words, the lookahead table and every slot of two snapshots
    byte-identical, the derived buffers CURRENT (poisoned through their zero-copy views, they read back poisoned), and the prepared next
    episodes untouched: the next 40 real steps under autoreset equal the oracle's."""
    import torch
    spec = T.build_spec(cfg)
    n, A, H, cap = 130, len(spec.actions_id), 12, 300
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed, autoreset=True, horizon=H)
    o = Oracle(spec.compile(), n, seed=seed, autoreset=True, horizon=H)
    v.reset(); o.reset()
    rs = np.random.RandomState(9)
    for t in range(7):
        a = rs.randint(0, A, n).astype(np.int32)
        v.step(a); o.step(a)
    pool, other = v.snapshot(cap), v.snapshot(n)
    pool.save(slots=np.arange(n)); other.save()
    table = v.key_table(4 * n * A)
    before = _everything(v, (pool, other))

    def kinds():
        v.successor_keys()
        v.successor_keys(rs.randint(0, n, 70), SK.ALL, reports=False)
        pool.successor_keys(fields=SK.POSE)
        other.successor_keys(dev_i32(rs.randint(0, n, 200)), device=True)
        pool.insert_successor_keys(table, rs.randint(0, cap, 90))
        v.insert_successor_keys(table, device=True)
    kinds()
    after = _everything(v, (pool, other))
    for k in before:
        assert before[k].dtype == after[k].dtype and (before[k] == after[k]).all(), k
    v.lookahead(device=True)['reward'].fill_(-77)                # both derived buffers poisoned through their zero-copy views
    v.action_mask_words(device=True).fill_(-1)
    torch.cuda.synchronize()
    kinds()
    assert (v.lookahead(copy=True)['reward'] == -77).all(), "a successor_keys call made the lookahead table stale"
    assert (v.action_mask_words(copy=True) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "a successor_keys call made the action masks stale"
    ends = 0
    for t in range(40):                                         # no prepared episode was consumed: the resets are the oracle's
        a = rs.randint(0, A, n).astype(np.int32)
        assert not o.step(a) & 2
        _, reward, done, _ = v.step(a, copy=True)
        assert (reward == o.reward).all() and (done == o.done.astype(bool)).all(), t
        ends += int(done.sum())
    s = v.get_state()
    for k, ref in zip(XO.STATE_KEYS, (o.st.map, o.st.loc, o.st.facing, o.st.inv, o.st.selected, o.st.step_count, o.st.episode)):
        assert (s[k].reshape(ref.shape) == ref).all(), k
    assert ends >= 2 * n
    assert v.error_flags() == 0
    v.close()


def test_bad_indices_in_a_device_list_give_rows_of_zeros():
    """One negative index, one equal to the capacity and one beyond it among good ones, count no multiple of 64: those rows are all zeros in
    every output, every other row is the oracles', F_BAD_INDEX is raised once, and nothing is stored outside [0, count * A) of any output -
    the guard values before and behind each are intact.  The same through the env rows (s == NULL)."""
    import torch
    spec = T.build_spec('axe10')
    n, A, cap = 70, len(spec.actions_id), 140
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    v.reset()
    rs = np.random.RandomState(8)
    for t in range(20):
        v.step(rs.randint(0, A, n).astype(np.int32))
    pool = v.snapshot(cap)
    pool.save(envs=rs.randint(0, n, cap), slots=np.arange(cap))
    count, pad = 130, 16
    bad_at = [5, 65, 129]
    for snap, limit, rows in ((pool, cap, pool.state()), (None, n, v.get_state())):
        idx = rs.randint(0, limit, count)
        idx[bad_at] = [-1, limit, 2 ** 31 - 1]
        exp = SKO.Successors(spec, rows, np.where(np.isin(np.arange(count), bad_at), 0, idx))
        d = dev_i32(idx)
        bufs = [torch.full((count * A + 2 * pad,), g, dtype=dt, device='cuda') for g, dt in
                ((0x5A5A5A5A5A5A5A5A, torch.int64), (0x5A5A5A5A, torch.int32), (0x5A, torch.uint8), (0x5A5A5A5A, torch.int32))]
        torch.cuda.synchronize()
        assert v.error_flags() == 0
        _cabi.check(_cabi.lib().ngw_successor_keys(v._h, snap._s if snap else None, C.c_void_p(d.data_ptr()), count, SK.ALL,
                                                   *[C.c_void_p(b.data_ptr() + pad * b.element_size()) for b in bufs]))
        v.sync()
        assert v.error_flags() == F_BAD_INDEX and v.error_flags() == 0
        host = [b.cpu().numpy() for b in bufs]
        for h, g in zip(host, (0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A, 0x5A5A5A5A)):
            assert (h[:pad] == g).all() and (h[pad + count * A:] == g).all(), "stores outside the count * A outputs"
        inner = [h[pad:pad + count * A].reshape(count, A) for h in host]
        got = SuccessorKeys(inner[0].view(np.uint64), inner[1], inner[2].view(np.bool_), (inner[3] & 1).astype(bool), inner[3].view(np.uint32))
        SKO.assert_successors(got, exp, SK.ALL, 'rows beside bad indices', zero_rows=bad_at)
        assert all((np.asarray(x)[bad_at] == 0).all() for x in got)
    s = pool.successor_keys(dev_i32([3, cap, 4]))                # the Python call: the same clamp
    assert (s.keys[1] == 0).all() and (s.info[1] == 0).all() and v.error_flags() == F_BAD_INDEX
    SKO.assert_successors(s, SKO.Successors(spec, pool.state(), [3, 0, 4]), SK.STATE, 'python call', zero_rows=[1])
    v.close()


def test_refusal_and_argument_errors():
    """The first map size beyond the limit - computed as the library computes it; 32 is inside - is refused with the message and the handle
    still steps and serves keys(); each NGW_E_INVALID_ARG case of include/ngw.h returns the code and launches nothing."""
    import torch
    L = _cabi.lib()
    K = len(make_spec(T.POGO, 10).items_id)
    first_beyond = next(S for S in range(10, 65) if lds_bytes(S, K) > LDS_MAX)
    assert lds_bytes(32, 24) <= LDS_MAX and lds_bytes(34, 24) <= LDS_MAX and lds_bytes(first_beyond - 1, K) <= LDS_MAX < lds_bytes(first_beyond, K)
    n = 70
    big = VecNovelGridworld(spec=make_spec(T.POGO, first_beyond), num_envs=n, seed=4)
    big.reset()
    bs = big.snapshot(n)
    bs.save()
    for call in (big.successor_keys, bs.successor_keys, lambda: bs.insert_successor_keys(big.key_table(64))):
        with pytest.raises(_cabi.NgwError, match=r'map_size %d: this call keeps two sets of a wavefront.s 64 maps in LDS \(ngw_successor_keys.*more than '
                                                 r'160 KiB; ngw_snapshot_expand followed by ngw_state_keys is available' % first_beyond):
            call()
    big.step(np.zeros(n, np.int32))                              # the handle still steps and serves keys
    SK.assert_keys(big.state_keys(), big.get_state(), np.arange(n), SK.STATE, 'beyond the limit: envs')
    SK.assert_keys(bs.keys(fields=SK.ALL), bs.state(), np.arange(n), SK.ALL, 'beyond the limit: slots')
    assert big.error_flags() == 0
    big.close()
    inside = VecNovelGridworld(spec=make_spec(T.POGO, first_beyond - 1), num_envs=3, seed=XO.good_seed(make_spec(T.POGO, first_beyond - 1), 3))
    inside.reset()                                               # the last size inside the limit is served
    SKO.assert_successors(inside.successor_keys(), SKO.Successors(inside.spec, inside.get_state(), np.arange(3)), SK.STATE, 'S=%d' % (first_beyond - 1))
    inside.close()
    spec = T.build_spec('pogo10')
    A = len(spec.actions_id)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    w = VecNovelGridworld(spec=spec, num_envs=n, seed=4)
    v.reset(); w.reset()
    s, foreign = v.snapshot(8), w.snapshot(8)
    s.save(slots=np.arange(8), envs=np.arange(8))
    buf = torch.full((n * A + 64,), 0x77, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    out, E, X = C.c_void_p(buf.data_ptr()), _cabi.E_INVALID_ARG, L.ngw_successor_keys
    none = (None, None, None)
    assert X(None, s._s, None, 8, 15, out, *none) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, s._s, None, 8, 15, None, *none) == E and 'NULL' in _cabi.last_error()
    assert X(v._h, foreign._s, None, 8, 15, out, *none) == E and 'not an open snapshot' in _cabi.last_error()
    for fields in (0, 64, 128, 1 << 31, 63 | 256):
        assert X(v._h, s._s, None, 8, fields, out, *none) == E and 'fields' in _cabi.last_error(), fields
    assert X(v._h, s._s, None, -1, 15, out, *none) == E and X(v._h, None, None, -1, 15, out, *none) == E
    assert X(v._h, s._s, None, 9, 15, out, *none) == E and '8 slots' in _cabi.last_error()        # no list: above the capacity
    assert X(v._h, None, None, n + 1, 15, out, *none) == E and '%d envs' % n in _cabi.last_error()  # ... above n_envs
    idx = dev_i32([0])
    assert X(v._h, s._s, C.c_void_p(idx.data_ptr()), (0x7FFFFFFF * 64) // A + 1, 15, out, *none) == E and 'actions' in _cabi.last_error()
    assert X(v._h, s._s, None, 0, 15, out, *none) == 0 and X(v._h, None, None, 0, 63, out, *none) == 0
    closed = v.snapshot(4)
    handle = closed._s
    closed.close()
    assert X(v._h, handle, None, 1, 15, out, *none) == E
    with pytest.raises(ValueError, match='closed'):
        closed.successor_keys()
    v.sync()
    assert (buf == 0x77).all()                                   # (nothing ran)
    for bad in (0, 64, -1, 1.5):
        with pytest.raises(ValueError, match='fields'):
            s.successor_keys(fields=bad)
        with pytest.raises(ValueError, match='fields'):
            v.successor_keys(fields=bad)
    with pytest.raises(ValueError):
        s.successor_keys([8])
    with pytest.raises(ValueError):
        v.successor_keys([n])
    with pytest.raises(ValueError, match='another env'):
        s.insert_successor_keys(w.key_table(8))
    assert s.successor_keys([]).keys.shape == (0, A) and v.successor_keys([]).reward.shape == (0, A)
    assert v.error_flags() == 0
    v.close(); w.close()


def _first_launch_is_successor_keys(S):
    """(child process) a fresh handle at map size S whose first launch after the reset's own is successor_keys, held to the oracles on 64 envs."""
    spec = make_spec(T.POGO, S)
    n = 64
    seed = XO.good_seed(spec, n)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=seed)
    v.reset()
    s = v.successor_keys(fields=SK.ALL)
    SKO.assert_successors(s, SKO.Successors(spec, v.get_state(), np.arange(n)), SK.ALL, 'S=%d, the first launch' % S)
    assert v.error_flags() == 0
    v.close()
    print('successor keys S=%d ok' % S, flush=True)


def test_the_lds_opt_in_in_a_fresh_process():
    """ONE child process whose first launch of any kernel that asks for more than 64 KiB of LDS is successor_keys, at S = 24 (above 64 KiB) and then S = 32 (a larger request from the same instantiation's table)."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, "the child failed:\n%s\n%s" % (out.stdout[-3000:], out.stderr[-3000:])
    for S in (24, 32):
        assert 'successor keys S=%d ok' % S in out.stdout, out.stdout


def _rows_of(children, at):
    return {k: np.asarray(children[k])[at].reshape(len(at), -1) if k in ('map', 'loc', 'inv') else np.asarray(children[k])[at] for k in XO.STATE_KEYS}


def test_breadth_first_search_closes_without_a_children_pool():
    """Five levels from one reset state of pogo10 with ONE archive pool and one table: per level insert_successor_keys over the frontier, then
    expand of exactly the fresh (parent, action) pairs into the next free archive slots.  Per level the set of new keys equals the one the
    existing loop finds (expand_all into a scratch pool, insert_keys, copy) and the one the CPU oracles find with a Python set; the archive
    never holds more rows than states discovered."""
    from gym_novel_gridworlds_amd.state_keys import keys_of_rows
    spec = T.build_spec('pogo10')
    v = VecNovelGridworld(spec=spec, num_envs=2, seed=XO.good_seed(spec, 2))
    v.reset()
    A, levels, room = v.n_actions, 5, 4096
    archive, table = v.snapshot(room), v.key_table(room)
    archive.save(envs=[0], slots=[0])
    keys, ins = archive.insert_keys(table, [0])
    assert ins.fresh.tolist() == [True]
    # the existing loop, beside it: its own archive, scratch pool and table
    old_archive, old_table = v.snapshot(room), v.key_table(room)
    old_archive.save(envs=[0], slots=[0])
    old_archive.insert_keys(old_table, [0])
    old_frontier, old_filled = np.array([0]), 1
    # the CPU side's root
    root = v.get_state()
    rows = _rows_of(root, [0])
    seen = {int(keys_of_rows(rows)[0])}
    assert int(keys[0]) in seen
    frontier, filled = np.array([0]), 1
    for level in range(1, levels + 1):
        P = len(frontier)
        s, found = archive.insert_successor_keys(table, frontier)
        assert found.fresh.shape == (P, A)
        j, a = fresh_pairs(found.fresh)
        new = len(j)
        assert filled + new <= room
        e = archive.expand(frontier[j], a, filled + np.arange(new))          # straight into the archive: exactly the new states
        assert (e.reward == s.reward[j, a]).all() and (e.info == s.info[j, a]).all() and (e.done == s.done[j, a]).all()
        new_keys = s.keys[j, a]
        assert (archive.keys(filled + np.arange(new)) == new_keys).all(), "level %d: an expanded child does not hold its announced key" % level
        frontier, filled = filled + np.arange(new), filled + new
        assert filled == len(table), "the archive holds exactly the states discovered"
        # the existing loop
        scratch = v.snapshot(len(old_frontier) * A)
        scratch.expand_all(old_frontier, 0, source=old_archive)
        okeys, oins = scratch.insert_keys(old_table, np.arange(len(old_frontier) * A))
        onew = np.nonzero(oins.fresh)[0]
        old_archive.copy(onew, old_filled + np.arange(len(onew)), source=scratch)
        old_frontier, old_filled = old_filled + np.arange(len(onew)), old_filled + len(onew)
        scratch.close()
        # the CPU oracles
        n_rows = len(rows['loc'])
        children, _ = XO.oracle_expand(spec, rows, np.repeat(np.arange(n_rows), A), np.tile(np.arange(A), n_rows))
        ckeys = SK.keys_of(children, range(n_rows * A), SK.STATE)
        fresh_cpu = []
        for pos, k in enumerate(ckeys.tolist()):
            if k not in seen:
                seen.add(k)
                fresh_cpu.append(pos)
        assert n_rows == P and (s.keys.reshape(-1) == ckeys).all(), "level %d: the children's keys differ" % level
        assert set(new_keys.tolist()) == set(okeys[onew].tolist()) == set(ckeys[fresh_cpu].tolist()) and new == len(onew) == len(fresh_cpu), level
        assert (j * A + a).tolist() == fresh_cpu == onew.tolist()
        rows = _rows_of(children, fresh_cpu)
        assert new > 0
    assert len(table) == len(old_table) == len(seen) == filled == old_filled
    held = archive.keys(np.arange(filled))
    assert len(set(held.tolist())) == filled and set(held.tolist()) == seen
    assert v.error_flags() == 0
    v.close()


def test_the_adapter_limit_actions_and_a_wrapper_forward():
    """The single-env adapter returns [A] fields that equal the oracles' for its state; LimitActions selects its own ids' columns, as its
    lookahead() does; a novelty wrapper forwards unchanged."""
    from gym_novel_gridworlds_amd import LimitActions
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    env = T.make_adapter_env('axe10', 'hip')
    env.reset()
    rs = np.random.RandomState(5)
    A = len(env.actions_id)
    for t in range(15):
        env.step(int(rs.randint(0, A)))
    vec = env.unwrapped._backend()                                # (the fixture env is the adapter under its novelty wrapper: a forward already)
    spec = vec.spec
    exp = SKO.Successors(spec, vec.get_state(), [0])
    s = env.successor_keys(SK.ALL)
    assert isinstance(s, SuccessorKeys) and all(x.shape == (A,) for x in s) and s.keys.dtype == np.uint64
    SKO.assert_successors(SuccessorKeys(*[x[None] for x in s]), exp, SK.ALL, 'adapter')
    look = env.lookahead(copy=True)
    assert (s.reward == look.reward).all() and (s.info == look.info).all()
    bare = env.successor_keys(reports=False)
    assert bare.reward is None and (bare.keys == exp.keys(SK.STATE)[0]).all()
    wrapped = NoveltyWrapper(env)
    assert all((x == y).all() for x, y in zip(wrapped.successor_keys(SK.ALL), s))
    names = sorted(env.actions_id)[::2]
    lim = LimitActions(env, set(names))
    ls, ll = lim.successor_keys(SK.ALL), lim.lookahead(copy=True)
    assert all(x.shape == (len(names),) for x in ls)
    for i, name in enumerate(sorted(names)):
        col = env.actions_id[name]
        assert all(x[i] == y[col] for x, y in zip(ls, s)), name
    assert (ls.reward == ll.reward).all() and (ls.info == ll.info).all() and (ls.done == ll.done).all()
    env.close()


if __name__ == '__main__':
    from oracle import ngw_oracle
    ngw_oracle.build()
    for size in (24, 32):
        _first_launch_is_successor_keys(size)
