"""tools/expand_cost.py - what expanding saved states into new slots costs (include/ngw.h ngw_snapshot_expand), one JSON line per map size.

    python tools/expand_cost.py [--n 65536] [--reps 20] [--rounds 5] [--cfgs C2,S32]

One child process per configuration (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32), each under its own time limit; the first one that
fails ends the run.  `n` pairs on a handle of `n` envs (the loop below cannot take more pairs than envs), autoreset off, the parents `n`
random slots of one snapshot (they repeat), the children a permutation of the slots of a second one, one random action per pair - all
device tensors.  After a warm-up, `rounds` rounds alternate the two variants; every figure is a HIP event pair on the env's stream around a
window of `reps` repetitions (the average INCLUDING the gaps between launches - what a caller's loop pays), reported as the median of the
rounds with their minimum and maximum:
    expand              ngw_snapshot_expand: one launch, no env touched
    restore_step_save   the loop it replaces: snapshot.restore(parents -> envs) + step_device + snapshot.save(envs -> children), three
                        launches (the restore restores the episode counters, as the expand's children carry their parents')
The tool asserts that the two leave the same children and reports.  No bar: the claim of the expand is one launch, no env touched and a
count not bound by num_envs, not a ratio."""
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
KEYS = ('map', 'loc', 'facing', 'inv', 'selected', 'step_count', 'episode')


def child(args):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    cfg, n = args.child, args.n
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    g = torch.Generator(device='cuda:0')
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device='cuda:0', generator=g)
    acts = torch.randint(0, A, (n,), dtype=torch.int32, device='cuda:0', generator=g)
    parents = torch.randint(0, n, (n,), dtype=torch.int32, device='cuda:0', generator=g)
    children = torch.randperm(n, device='cuda:0', generator=g).to(torch.int32)
    reward = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    done = torch.zeros(n, dtype=torch.uint8, device='cuda:0')
    info = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    src, dst_e, dst_l = v.snapshot(), v.snapshot(), v.snapshot()
    src.save()
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def expand():
        _cabi.check(L.ngw_snapshot_expand(v._h, src._s, ptr(parents), ptr(acts), dst_e._s, ptr(children), n, ptr(reward), ptr(done), ptr(info)))

    def restore_step_save():
        src.restore(slots=parents)
        v.step_device(acts.data_ptr())
        dst_l.save(slots=children)
    variants = {'expand': expand, 'restore_step_save': restore_step_save}
    res = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(2):
            fn()
    v.sync()
    for r in range(args.rounds):
        for k, fn in variants.items():
            v.timing_begin()
            for _ in range(args.reps):
                fn()
            res[k].append(v.timing_end() * 1e3 / args.reps)
    # ---- the two answers agree
    expand()
    restore_step_save()
    v.sync()
    a, b = dst_e.state(), dst_l.state()
    for k in KEYS:
        assert (a[k] == b[k]).all(), (cfg, k)
    out3 = v.device_outputs()
    torch.cuda.synchronize()
    assert bool((reward == out3['reward']).all()) and bool((done == out3['done'].view(torch.uint8)).all()), (cfg, 'reports')
    assert bool((info == out3['info'].view(torch.int32)).all()), (cfg, 'info')
    assert v.error_flags() == 0
    out = {'figure': 'expand_cost', 'cfg': cfg, 'n': n, 'S': S, 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'ended': round(float(done.float().mean()), 4)}
    for k, x in res.items():
        out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    out['loop_over_expand'] = round(out['restore_step_save']['us'] / out['expand']['us'], 2)
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--limit', type=int, default=180, help='seconds per configuration')
    ap.add_argument('--child', default='')
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', str(a.n),
                              '--reps', str(a.reps), '--rounds', str(a.rounds)])
        if rc:
            print(json.dumps({'figure': 'expand_cost', 'cfg': cfg, 'failed': rc}), flush=True)
            sys.exit(rc)
