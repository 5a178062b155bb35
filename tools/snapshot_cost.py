"""tools/snapshot_cost.py - what device-side snapshots cost (include/ngw.h ngw_snapshot_*), one JSON line per configuration.

    python tools/snapshot_cost.py [--n 65536] [--reps 200] [--rounds 5] [--cfgs C2,C3,C5]

One child process per configuration (C2 Pogostick-v1 10 x 10, C3 Bow-v1 20 x 20, C5 AddItem 32 x 32), each under its own time limit; the
first one that fails ends the run.  Per configuration, after a warm-up, `rounds` rounds that alternate the variants; every device figure
is a HIP event pair on the env's stream around `reps` repetitions:
    save_all            slot i := env i                       restore_identity    env i := slot i
    restore_permuted    env i := slot perm[i]                 restore_fanout64    env i := slot i % 64 (a fork fan-out)
    save_all_copies / restore_identity_copies                 the two contiguous cases as seven device-to-device copies (NGW_SNAP_MEMCPY=1)
    host_round_trip     get_state() + set_state() of all envs, wall clock (code this change does not touch)
    step                step_device alone                     restore_step / restore_keep_step   restore (identity) + step_device
For each: microseconds (median and min-max over the rounds), bytes moved = 2 * count * (S*S + 4*K + 21) (+ 4 per index read), bytes per
second and that as a share of the 8.0 TB/s HBM peak."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10, None), 'C3': ('NovelGridworld-Bow-v1', 20, None),
       'C5': ('NovelGridworld-Pogostick-v1', 32, ('additem', 'hard', 'arrow', ''))}
HBM_PEAK = 8.0e12


def make(cfg, n):
    from gym_novel_gridworlds_amd import VecNovelGridworld, apply_novelty, make_spec
    env_id, S, nov = CFG[cfg]
    spec = make_spec(env_id, S)
    if nov:
        apply_novelty(spec, *nov)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1, autoreset=True, horizon=100)
    v.reset()
    return v


def child(args):
    import torch
    cfg, n = args.child, args.n
    v = make(cfg, n)
    os.environ['NGW_SNAP_MEMCPY'] = '1'                   # (read when a snapshot is created: this handle's contiguous copies are hipMemcpyAsync)
    vc = make(cfg, n)
    sc = vc.snapshot()
    os.environ.pop('NGW_SNAP_MEMCPY')
    s = v.snapshot()
    S2, K, A = v.map_size ** 2, v.n_items, len(v.actions_id)
    row = S2 + 4 * K + 21
    acts = torch.randint(0, A, (64, n), dtype=torch.int32, device='cuda:0')
    rs = np.random.RandomState(0)
    perm = torch.from_numpy(rs.permutation(n).astype(np.int32)).to('cuda:0')
    fan = torch.from_numpy((np.arange(n) % 64).astype(np.int32)).to('cuda:0')
    torch.cuda.synchronize()
    for t in range(40):
        v.step_device(acts[t % 64].data_ptr()); vc.step_device(acts[t % 64].data_ptr())
    s.save(); sc.save()
    v.sync(); vc.sync()
    step_i = [0]

    def step(e):
        e.step_device(acts[step_i[0] % 64].data_ptr())
        step_i[0] += 1
    variants = {
        'save_all': (v, lambda: s.save(), 2 * n * row),
        'restore_identity': (v, lambda: s.restore(), 2 * n * row),
        'restore_permuted': (v, lambda: s.restore(slots=perm), 2 * n * row + 4 * n),
        'restore_fanout64': (v, lambda: s.restore(slots=fan), 2 * n * row + 4 * n),
        'save_all_copies': (vc, lambda: sc.save(), 2 * n * row),
        'restore_identity_copies': (vc, lambda: sc.restore(), 2 * n * row),
        'step': (v, lambda: step(v), None),
        'restore_step': (v, lambda: (s.restore(), step(v)), None),
        'restore_keep_step': (v, lambda: (s.restore(keep_episode=True), step(v)), None),
    }
    res = {k: [] for k in variants}
    res['host_round_trip'] = []

    def host_round_trip():
        st = v.get_state()
        v.set_state(0, **st)
    for k, (e, fn, _) in variants.items():               # warm-up of every shape the timed windows use
        for _ in range(10):
            fn()
        e.sync()
    host_round_trip()
    for r in range(args.rounds):
        for k, (e, fn, _) in variants.items():
            e.sync()
            e.timing_begin()
            for _ in range(args.reps):
                fn()
            res[k].append(e.timing_end() * 1e3 / args.reps)
        v.sync()
        t0 = time.perf_counter()
        for _ in range(3):
            host_round_trip()
        res['host_round_trip'].append((time.perf_counter() - t0) / 3 * 1e6)
        s.save(); v.sync()                                # (set_state and the steps moved the state on: the next round restores a fresh save)
    assert v.error_flags() == 0 and vc.error_flags() == 0
    out = {'figure': 'snapshot_cost', 'cfg': cfg, 'n': n, 'S': v.map_size, 'K': K, 'row_bytes': row, 'reps': args.reps, 'rounds': args.rounds}
    for k, x in res.items():
        b = variants[k][2] if k in variants else 2 * n * row
        d = {'us': round(float(np.median(x)), 2), 'min': round(float(min(x)), 2), 'max': round(float(max(x)), 2)}
        if b:
            d['bytes'] = b
            d['GBps'] = round(b / (np.median(x) * 1e-6) / 1e9, 1)
            d['hbm_share'] = round(b / (np.median(x) * 1e-6) / HBM_PEAK, 4)
        out[k] = d
    dev = out['save_all']['us'] + out['restore_identity']['us']
    spread = max(out['save_all']['max'] - out['save_all']['min'] + out['restore_identity']['max'] - out['restore_identity']['min'],
                 out['host_round_trip']['max'] - out['host_round_trip']['min'])
    out['device_save_plus_restore_us'] = round(dev, 2)
    out['bar_device_faster_than_host_by_more_than_the_spread'] = bool(out['host_round_trip']['us'] - dev > spread)
    print(json.dumps(out), flush=True)
    v.close(); vc.close()
    if not out['bar_device_faster_than_host_by_more_than_the_spread']:
        sys.exit(3)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,C3,C5')
    ap.add_argument('--limit', type=int, default=240, help='seconds per configuration')
    ap.add_argument('--child', default='')
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', str(a.n),
                              '--reps', str(a.reps), '--rounds', str(a.rounds)])
        if rc:
            print(json.dumps({'figure': 'snapshot_cost', 'cfg': cfg, 'failed': rc}), flush=True)
            sys.exit(rc)
