"""tools/walk_cost.py - what walk distances and go-to plans cost (include/ngw.h ngw_snapshot_walk), one JSON line per map size and count.

    python tools/walk_cost.py [--counts 4096,65536] [--reps 10] [--rounds 5] [--cfgs C2,S32] [--steps 64]

One child process per (configuration, count) (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32), each under its own time limit; the first one
that fails ends the run.  `count` slots of one snapshot on a handle of `count` envs (after 20 random steps), walked through a random slot list
with repeats - a device tensor - into buffers allocated once; every row asks for tree_log.  After a warm-up, `rounds` rounds alternate the
device variants; each figure is a HIP event pair on the env's stream around a window of `reps` calls (the average INCLUDING the gaps between
launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    walk_dist      ngw_snapshot_walk without items: the layers and the per-id minima, K distances per row
    walk_plans     ... with items and T = --steps: also the walk back and the [T][count] plans
    keys_state     the yardstick: ngw_state_keys of the same slots - a kernel that reads the same rows and does next to nothing with them
    host_loop      the loop the call replaces, in wall time: pool.state() to the host, walk.shortest_walks (numpy, in chunks of 4096 rows), the
                   plans uploaded and the device synchronised.  Its rounds are --host-rounds (default: `rounds` up to 4096 rows, 1 above - one
                   round of 65 536 rows takes the better part of a minute).
The breadth-first depth drives the kernel's time, so the line carries the layer count of the deepest row and the mean over the rows (from the
host twin, over up to 4096 sampled rows).  The tool checks 64 random rows against the host twin.  No bar is set."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}
CHUNK = 4096


def child(args):
    import torch
    from gym_novel_gridworlds_amd import KEY_STATE, VecNovelGridworld, _cabi, make_spec
    from gym_novel_gridworlds_amd.walk import shortest_walks, walk_fields
    cfg, n, T = args.child, args.n, args.steps
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A, item = len(spec.actions_id), spec.items_id['tree_log']
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    slots = torch.randint(0, n, (n,), dtype=torch.int32, device=dev, generator=g)
    items = torch.full((n,), item, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    K = v.n_items
    dist = torch.zeros((n, K), dtype=torch.int32, device=dev)
    plans = torch.zeros((T, n), dtype=torch.int32, device=dev)
    length = torch.zeros(n, dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    pool = v.snapshot()
    pool.save()                                            # the nodes
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    variants = {'walk_dist': lambda: _cabi.check(L.ngw_snapshot_walk(v._h, pool._s, ptr(slots), n, None, 0, ptr(dist), None, None)),
                'walk_plans': lambda: _cabi.check(L.ngw_snapshot_walk(v._h, pool._s, ptr(slots), n, ptr(items), T, ptr(dist), ptr(plans), ptr(length))),
                'keys_state': lambda: _cabi.check(L.ngw_state_keys(v._h, pool._s, ptr(slots), n, KEY_STATE, ptr(keys)))}
    out = {'figure': 'walk_cost', 'cfg': cfg, 'n': n, 'S': S, 'T': T, 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
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
    idx = slots.cpu().numpy()
    item_ids = np.full(n, item, np.int32)

    def host_loop():
        rows = pool.state()
        got = []
        for first in range(0, n, CHUNK):
            at = idx[first:first + CHUNK]
            got.append(shortest_walks({k: rows[k][at] for k in ('map', 'loc', 'facing')}, item_ids[first:first + CHUNK], T, spec))
        up = torch.from_numpy(np.ascontiguousarray(np.concatenate([w.plans for w in got], axis=1))).to(dev)
        torch.cuda.synchronize()
        return got, up
    host_rounds = args.host_rounds or (args.rounds if n <= 4096 else 1)
    wall = []
    for r in range(host_rounds):
        t0 = time.perf_counter()
        got, up = host_loop()
        wall.append((time.perf_counter() - t0) * 1e6)
    out['host_loop'] = {'us': round(float(np.median(wall)), 1), 'min': round(float(min(wall)), 1), 'max': round(float(max(wall)), 1), 'rounds': host_rounds}
    for k in ('walk_dist', 'walk_plans'):
        out[k + '_over_keys'] = round(out[k]['us'] / out['keys_state']['us'], 2)
    out['host_loop_over_walk_plans'] = round(out['host_loop']['us'] / out['walk_plans']['us'], 1)
    # the layers (of up to 4096 sampled rows), and the answers of 64 random positions against the host twin
    rows = pool.state()
    some = np.random.RandomState(5).choice(n, min(n, CHUNK), replace=False)
    D, _ = walk_fields(rows['map'][some], rows['loc'][some], rows['facing'][some])
    depth = D.reshape(len(D), -1).max(1)
    out['layers_max'], out['layers_mean'] = int(depth.max()), round(float(depth.mean()), 1)
    variants['walk_plans']()
    v.sync()
    at = np.random.RandomState(3).randint(0, n, 64)
    want_p = np.concatenate([w.plans for w in got], axis=1)[:, at]
    want_l, want_d = np.concatenate([w.length for w in got])[at], np.concatenate([w.dist for w in got])[at]
    assert (plans.cpu().numpy()[:, at] == want_p).all() and (length.cpu().numpy()[at] == want_l).all() and (dist.cpu().numpy()[at] == want_d).all(), cfg
    out['reached'] = round(float((length.cpu().numpy() >= 0).mean()), 3)
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=0)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--limit', type=int, default=400, help='seconds per child')
    ap.add_argument('--child', default='')
    ap.add_argument('--n', type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        for n in a.counts.split(','):
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', n,
                                  '--reps', str(a.reps), '--rounds', str(a.rounds), '--steps', str(a.steps), '--host-rounds', str(a.host_rounds)])
            if rc:
                print(json.dumps({'figure': 'walk_cost', 'cfg': cfg, 'n': int(n), 'failed': rc}), flush=True)
                sys.exit(rc)
