"""tools/key_cost.py - what device-side state keys cost (include/ngw.h ngw_state_keys), one JSON line per map size and count.

    python tools/key_cost.py [--counts 4096,65536] [--reps 10] [--rounds 5] [--cfgs C2,S32]

One child process per (configuration, count) (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32), each under its own time limit; the first one
that fails ends the run.  `count` slots of one snapshot on a handle of `count` envs, keyed through a random slot list with repeats - a device
tensor - into a buffer allocated once.  After a warm-up, `rounds` rounds alternate the variants; every figure is a HIP event pair on the env's
stream around a window of `reps` calls (the average INCLUDING the gaps between launches - what a caller's loop pays), reported as the median of
the rounds with their minimum and maximum:
    keys_state / keys_all      ngw_state_keys under NGW_KEY_STATE / NGW_KEY_ALL: reads the rows, writes 8 B per row
    save                       the yardstick: snap.save() of the same count on the same handle - reads the same rows, writes the rows
    save_gather                the same copy through a random env list with repeats into slots 0 .. count-1 (reads gathered like the key call's)
The tool checks the keys of 64 random rows against the host twin (state_keys.keys_of_rows) and reports us per call, bytes moved per row and the
ratio key call / save.  No bar is set."""
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
    from gym_novel_gridworlds_amd import KEY_ALL, KEY_STATE, VecNovelGridworld, _cabi, keys_of_rows, make_spec
    cfg, n = args.child, args.n
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    slots = torch.randint(0, n, (n,), dtype=torch.int32, device=dev, generator=g)
    every = torch.arange(n, dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    K = v.n_items
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    pool, copy = v.snapshot(), v.snapshot()
    pool.save()                                            # the nodes
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def keyed(fields):
        return lambda: _cabi.check(L.ngw_state_keys(v._h, pool._s, ptr(slots), n, fields, ptr(keys)))
    variants = {'keys_state': keyed(KEY_STATE), 'keys_all': keyed(KEY_ALL),
                'save': lambda: _cabi.check(L.ngw_snapshot_save(v._h, copy._s, None, None, n)),
                'save_gather': lambda: _cabi.check(L.ngw_snapshot_save(v._h, copy._s, ptr(slots), ptr(every), n))}
    out = {'figure': 'key_cost', 'cfg': cfg, 'n': n, 'S': S, 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
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
    row = S * S + 4 * K + 8 + 4 + 1                         # map, inventory, location, facing, selected item
    out['keys_state']['B_per_row'] = row + 4 + 8            # (+ the index, + the key)
    out['keys_all']['B_per_row'] = row + 8 + 4 + 8          # (+ step count and episode counter)
    out['save']['B_per_row'] = 2 * (row + 8)
    out['save_gather']['B_per_row'] = 2 * (row + 8) + 8
    for k in ('keys_state', 'keys_all'):
        out[k + '_over_save'] = round(out[k]['us'] / out['save']['us'], 2)
        out[k + '_over_save_gather'] = round(out[k]['us'] / out['save_gather']['us'], 2)
    # the keys are the contract's (64 random positions, both selections, against the host twin)
    rows, at = pool.state(), np.random.RandomState(3).randint(0, n, 64)
    idx = slots.cpu().numpy()
    for fields in (KEY_STATE, KEY_ALL):
        keyed(fields)()
        v.sync()
        got = keys.cpu().numpy().view(np.uint64)[at]
        assert (got == keys_of_rows({k: x[idx[at]] for k, x in rows.items()}, fields)).all(), (cfg, fields)
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--limit', type=int, default=120, help='seconds per child')
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
                print(json.dumps({'figure': 'key_cost', 'cfg': cfg, 'n': int(n), 'failed': rc}), flush=True)
                sys.exit(rc)
