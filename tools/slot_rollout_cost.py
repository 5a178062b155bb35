"""tools/slot_rollout_cost.py - what rolling action sequences out from saved states costs (include/ngw.h ngw_snapshot_rollout), one JSON line
per map size and plan length.

    python tools/slot_rollout_cost.py [--n 65536] [--reps 10] [--rounds 5] [--cfgs C2,S32] [--steps 8,32]

One child process per configuration (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32) and plan length T, each under its own time limit;
the first one that fails ends the run.  `n` pairs on a handle of `n` envs (variant b cannot take more pairs than envs), autoreset off, the
parents `n` random slots of one snapshot (they repeat), the children a permutation of the slots of a second one, T random actions per pair -
all device tensors.  After a warm-up, `rounds` rounds alternate the three variants; every figure is a HIP event pair on the env's stream
around a window of `reps` repetitions (the average INCLUDING the gaps between launches - what a caller's loop pays), reported as the median
of the rounds with their minimum and maximum:
    rollout             (a) ngw_snapshot_rollout keeping the end state: one launch, no env touched
    restore_roll_save   (b) the loop it replaces: snapshot.restore(parents -> envs, keep_episode) + rollout_actions with reward / done rows +
                        the reduction in torch (sum of the rewards up to the first done, length, ended) + snapshot.save(envs -> children)
    chained_expands     (c) T ngw_snapshot_expand calls through two scratch snapshots, the last one into the children
The tool asserts that the three agree: ret / length / ended of every pair (and the last info word between a and c), and the kept rows of
every pair that did not end before its last step (b and c go on stepping an ended state - the sticky done -, a keeps the state the episode
ended in; the share of such pairs is reported as `ended_early`).  No bar: the comparison is against (b) and (c) on the same build."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}
KEYS = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count')


def child(args):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    cfg, n, T = args.child, args.n, args.t
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    plans = torch.randint(0, A, (T, n), dtype=torch.int32, device=dev, generator=g)
    parents = torch.randint(0, n, (n,), dtype=torch.int32, device=dev, generator=g)
    children = torch.randperm(n, device=dev, generator=g).to(torch.int32)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)   # noqa: E731
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dev)    # noqa: E731
    ret_a, len_a, end_a, info_a = i32(n), i32(n), u8(n), i32(n)
    rew_b, done_b = i32(T, n), u8(T, n)
    rew_c, done_c, info_c = i32(T, n), u8(T, n), i32(T, n)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    src, dst_a, dst_b, dst_c, tmp = v.snapshot(), v.snapshot(), v.snapshot(), v.snapshot(), (v.snapshot(), v.snapshot())
    src.save()
    v.rollout_outputs(rew_b.data_ptr(), done_b.data_ptr(), n)
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    red = {}

    def reduce(rew, done):
        """ret / length / ended of [T, n] reward and done rows: what counts is every step up to and including the first done."""
        d = done.to(torch.int32)
        before = torch.cumsum(d, 0) - d == 0                    # no done before step t
        return (rew * before).sum(0, dtype=torch.int32), before.sum(0, dtype=torch.int32), d.sum(0) > 0, before

    def rollout():
        _cabi.check(L.ngw_snapshot_rollout(v._h, src._s, ptr(parents), ptr(plans), n, T, dst_a._s, ptr(children), n, ptr(ret_a), ptr(len_a),
                                           ptr(end_a), ptr(info_a)))

    def restore_roll_save():
        src.restore(slots=parents, keep_episode=True)
        v.rollout_actions(plans.data_ptr(), n, T)
        v.stream_order(torch.cuda.current_stream(0).cuda_stream, False)      # the reduction runs on torch's stream, behind the rollout
        red['b'] = reduce(rew_b, done_b)
        v.stream_order(torch.cuda.current_stream(0).cuda_stream, True)
        dst_b.save(slots=children)

    def chained_expands():
        for t in range(T):
            s = src if t == 0 else tmp[(t + 1) % 2]
            d = dst_c if t == T - 1 else tmp[t % 2]
            _cabi.check(L.ngw_snapshot_expand(v._h, s._s, ptr(parents) if t == 0 else None, ptr(plans[t]), d._s, ptr(children) if t == T - 1 else None, n,
                                              ptr(rew_c[t]), ptr(done_c[t]), ptr(info_c[t])))
    variants = {'rollout': rollout, 'restore_roll_save': restore_roll_save, 'chained_expands': chained_expands}
    res = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(2):
            fn()
    v.sync()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for k, fn in variants.items():
            v.timing_begin()
            for _ in range(args.reps):
                fn()
            res[k].append(v.timing_end() * 1e3 / args.reps)
    # ---- the three answers agree
    for fn in variants.values():
        fn()
    v.sync()
    torch.cuda.synchronize()
    ret_b, len_b, end_b, _ = red['b']
    ret_c, len_c, end_c, before_c = reduce(rew_c, done_c)
    last = (len_c - 1).long().unsqueeze(0)
    for name, (r_, l_, e_) in {'b': (ret_b, len_b, end_b), 'c': (ret_c, len_c, end_c)}.items():
        assert bool((ret_a == r_).all()) and bool((len_a == l_).all()) and bool((end_a.bool() == e_).all()), (cfg, T, name, 'reports')
    assert bool((info_a == info_c.gather(0, last)[0]).all()), (cfg, T, 'info')
    early = (end_a.bool() & (len_a < T)).cpu().numpy()
    kept = children.cpu().numpy()[~early]
    a, b, c = dst_a.state(), dst_b.state(), dst_c.state()
    for k in KEYS:
        assert (a[k][kept] == b[k][kept]).all() and (a[k][kept] == c[k][kept]).all(), (cfg, T, k)
    assert v.error_flags() == 0
    out = {'figure': 'slot_rollout_cost', 'cfg': cfg, 'n': n, 'S': S, 'T': T, 'reps': args.reps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0), 'ended_early': round(float(early.mean()), 4)}
    for k, x in res.items():
        out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--steps', default='8,32')
    ap.add_argument('--limit', type=int, default=240, help='seconds per configuration and plan length')
    ap.add_argument('--child', default='')
    ap.add_argument('--t', type=int, default=8)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        for t in a.steps.split(','):
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--t', t, '--n', str(a.n),
                                  '--reps', str(a.reps), '--rounds', str(a.rounds)])
            if rc:
                print(json.dumps({'figure': 'slot_rollout_cost', 'cfg': cfg, 'T': int(t), 'failed': rc}), flush=True)
                sys.exit(rc)
