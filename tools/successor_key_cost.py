"""tools/successor_key_cost.py - what successor keys cost (include/ngw.h ngw_successor_keys) against the loop they replace, one JSON line per map
size and count.

    python tools/successor_key_cost.py [--counts 4096,65536] [--reps 10] [--rounds 5] [--cfgs C2,S32]

One child process per (configuration, count) (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32), each under its own time limit; the first one
that fails ends the run.  `count` parents: the slots of one snapshot on a handle of `count` envs after 20 random steps, taken through a random
slot list with repeats - a device tensor - into buffers allocated once.  After a warm-up, `rounds` rounds alternate the variants; every figure
is a HIP event pair on the env's stream around a window of `reps` calls (the average INCLUDING the gaps between launches - what a caller's loop
pays), reported as the median of the rounds with their minimum and maximum:
    succ / succ_keys_only    ngw_successor_keys under NGW_KEY_STATE with / without the three report arrays: reads the parents' rows, writes
                             8 (+ 9) bytes per (parent, action)
    loop                     the route it replaces, in the same window: ngw_snapshot_expand of the same parents with every action into a scratch
                             pool of count * A slots (with its reports), then ngw_state_keys of the count * A children
    loop_expand / loop_keys  the two calls of that route alone
The tool checks the keys and reports of the two routes against each other (every pair), reports us per call, the bytes each route moves per
parent, the scratch-pool bytes the loop needs, and loop / succ.  No bar is set."""
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


def child(args):
    import torch
    from gym_novel_gridworlds_amd import KEY_STATE, VecNovelGridworld, _cabi, make_spec
    cfg, n = args.child, args.n
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    parents = torch.randint(0, n, (n,), dtype=torch.int32, device=dev, generator=g)
    pairs = torch.arange(n * A, dtype=torch.int32, device=dev)
    pair_parent = parents.repeat_interleave(A).contiguous()
    pair_action = (pairs % A).contiguous()
    new = lambda dt: torch.zeros(n * A, dtype=dt, device=dev)   # noqa: E731
    keys, reward, done, info = new(torch.int64), new(torch.int32), new(torch.uint8), new(torch.int32)
    keys2, reward2, done2, info2 = new(torch.int64), new(torch.int32), new(torch.uint8), new(torch.int32)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    K = v.n_items
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    pool, scratch = v.snapshot(), v.snapshot(n * A)
    pool.save()                                            # the nodes
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def succ(reports):
        rep = (ptr(reward), ptr(done), ptr(info)) if reports else (None, None, None)
        return lambda: _cabi.check(L.ngw_successor_keys(v._h, pool._s, ptr(parents), n, KEY_STATE, ptr(keys), *rep))

    def expand():
        _cabi.check(L.ngw_snapshot_expand(v._h, pool._s, ptr(pair_parent), ptr(pair_action), scratch._s, None, n * A, ptr(reward2), ptr(done2), ptr(info2)))

    def child_keys():
        _cabi.check(L.ngw_state_keys(v._h, scratch._s, None, n * A, KEY_STATE, ptr(keys2)))

    def loop():
        expand()
        child_keys()
    variants = {'succ': succ(True), 'succ_keys_only': succ(False), 'loop': loop, 'loop_expand': expand, 'loop_keys': child_keys}
    out = {'figure': 'successor_key_cost', 'cfg': cfg, 'n': n, 'S': S, 'A': A, 'reps': args.reps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0)}
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
    v.sync()
    for k, x in res.items():
        out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    row = S * S + 4 * K + 8 + 4 + 1 + 4 + 4                 # map, inventory, location, facing, selected item, step count, episode counter
    out['succ']['B_per_parent'] = row + 4 + A * (8 + 9)     # the parent's row and index in, a key and the reports per action out
    out['succ_keys_only']['B_per_parent'] = row + 4 + A * 8
    out['loop_expand']['B_per_parent'] = A * (row + 4 + 4 + row + 9)    # per pair: the parent's row, its index and the action in, the child and the reports out
    out['loop_keys']['B_per_parent'] = A * (row - 8 + 8)    # per pair: the child's row (without the two counters) in, a key out
    out['loop']['B_per_parent'] = out['loop_expand']['B_per_parent'] + out['loop_keys']['B_per_parent']
    out['loop_scratch_pool_B'] = n * A * row
    out['loop_over_succ'] = round(out['loop']['us'] / out['succ']['us'], 2)
    out['loop_over_succ_keys_only'] = round(out['loop']['us'] / out['succ_keys_only']['us'], 2)
    out['faster_by_more_than_the_spread'] = bool(out['succ']['max'] < out['loop']['min'])
    # the two routes agree, pair for pair
    succ(True)()
    loop()
    v.sync()
    assert (keys == keys2).all() and (reward == reward2).all() and (done == done2).all() and (info == info2).all(), cfg
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--limit', type=int, default=150, help='seconds per child')
    ap.add_argument('--child', default='')
    ap.add_argument('--n', type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        for n in a.counts.split(','):
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', n,
                                  '--reps', str(a.reps), '--rounds', str(a.rounds)])
            if rc:
                print(json.dumps({'figure': 'successor_key_cost', 'cfg': cfg, 'n': int(n), 'failed': rc}), flush=True)
                sys.exit(rc)
