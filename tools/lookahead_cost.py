"""tools/lookahead_cost.py - what a one-step lookahead table costs (include/ngw.h ngw_lookahead), one JSON line per configuration.

    python tools/lookahead_cost.py [--n 65536] [--reps 50] [--rounds 5] [--cfgs C2,C3,C5]

One child process per configuration (C2 Pogostick-v1 10 x 10, C3 Bow-v1 20 x 20, C5 AddItem 32 x 32), each under its own time limit; the
first one that fails ends the run.  Per configuration, after a warm-up, `rounds` rounds that alternate the variants; every figure is a HIP
event pair on the env's stream around `reps` repetitions (a window of tens of launches: the event pair's own ~microseconds of jitter and the
gaps between launches are spread over it, and the figure is the average launch INCLUDING its gap - what a caller's loop pays):
    lookahead           ngw_lookahead alone.  A query on a current table launches nothing, so every repetition first changes the horizon
                        (100 <-> 101: a host-side setting, no device work) - the table is then recomputed under the other setting
    mask                the standalone mask kernel, for scale: step_device + ngw_action_mask (masks off) minus step_device alone
    step                step_device alone
    snapshot_loop       what a user runs without the table: snapshot.save() once, then for every action restore(keep_episode=True) +
                        step_device (that action for every env) + device-side copies of reward / done / info into a table [A, n].  The loop
                        runs code this change does not touch, so the same build stands for the parent here.
For the table: bytes moved = n * (S*S cells are NOT all read: <= 33 cells + 4*K + 17 B of state) + 9 * A * n written, bytes per second and
that as a share of the 8.0 TB/s HBM peak.  The bar: lookahead beats snapshot_loop by more than the spread (max - min) of either side."""
import argparse
import json
import os
import subprocess
import sys

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
    from gym_novel_gridworlds_amd import _cabi
    cfg, n = args.child, args.n
    L = _cabi.lib()
    v = make(cfg, n)
    K, A = v.n_items, len(v.actions_id)
    acts = torch.randint(0, A, (64, n), dtype=torch.int32, device='cuda:0')
    same = torch.arange(A, dtype=torch.int32, device='cuda:0')[:, None].repeat(1, n).contiguous()   # row a: action a for every env
    torch.cuda.synchronize()
    for t in range(40):
        v.step_device(acts[t % 64].data_ptr())
    s = v.snapshot()
    s.save()
    out3 = v.device_outputs()
    table = {k: torch.zeros((A, n), dtype=out3[k].dtype, device='cuda:0') for k in out3}
    v.sync()
    ts = torch.cuda.Stream()                              # the env and the loop's torch copies share ONE stream: ordered without a host wait
    v.set_stream(ts.cuda_stream)
    step_i, hz = [0], [0]

    def step():
        v.step_device(acts[step_i[0] % 64].data_ptr())
        step_i[0] += 1

    def lookahead():
        hz[0] ^= 1
        _cabi.check(L.ngw_set_autoreset(v._h, 1, 100 + hz[0]))
        _cabi.check(L.ngw_lookahead(v._h))

    def step_mask():
        step()
        _cabi.check(L.ngw_action_mask(v._h))

    def snapshot_loop():
        for a in range(A):
            s.restore(keep_episode=True)
            v.step_device(same[a].data_ptr())
            with torch.cuda.stream(ts):
                for k in table:
                    table[k][a].copy_(out3[k], non_blocking=True)
    variants = {'lookahead': (lookahead, args.reps), 'step': (step, args.reps), 'step_mask': (step_mask, args.reps),
                'snapshot_loop': (snapshot_loop, max(1, args.reps // 10))}
    res = {k: [] for k in variants}
    for k, (fn, reps) in variants.items():               # warm-up of every shape the timed windows use
        for _ in range(3):
            fn()
        v.sync()
    for r in range(args.rounds):
        for k, (fn, reps) in variants.items():
            s.restore(); v.sync()                         # every window starts from the saved state
            v.timing_begin()
            for _ in range(reps):
                fn()
            res[k].append(v.timing_end() * 1e3 / reps)
    _cabi.check(L.ngw_set_autoreset(v._h, 1, 100))
    assert v.error_flags() == 0
    # the loop's table and the kernel's agree (same state, same setting): the two variants time the same answer
    s.restore()
    snapshot_loop()
    s.restore()
    look = v.lookahead(device=True)
    torch.cuda.synchronize()
    assert bool((look['reward'].t() == table['reward']).all()) and bool((look['done'].t() == table['done'].bool()).all())
    assert bool((look['info'].t() == table['info']).all())
    S2 = v.map_size ** 2
    read = n * (min(S2, 33) + 4 * K + 17)
    moved = read + 9 * A * n
    out = {'figure': 'lookahead_cost', 'cfg': cfg, 'n': n, 'S': v.map_size, 'K': K, 'A': A, 'reps': args.reps, 'rounds': args.rounds,
           'bytes': moved}
    res['mask'] = [b - a for a, b in zip(res['step'], res['step_mask'])]
    for k, x in res.items():
        out[k] = {'us': round(float(np.median(x)), 2), 'min': round(float(min(x)), 2), 'max': round(float(max(x)), 2)}
    la, lo = out['lookahead'], out['snapshot_loop']
    la['GBps'] = round(moved / (la['us'] * 1e-6) / 1e9, 1)
    la['hbm_share'] = round(moved / (la['us'] * 1e-6) / HBM_PEAK, 4)
    spread = max(la['max'] - la['min'], lo['max'] - lo['min'])
    out['loop_over_lookahead'] = round(lo['us'] / la['us'], 1)
    out['bar_lookahead_beats_the_loop_by_more_than_the_spread'] = bool(lo['us'] - la['us'] > spread)
    print(json.dumps(out), flush=True)
    v.close()
    if not out['bar_lookahead_beats_the_loop_by_more_than_the_spread']:
        sys.exit(3)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=50)
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
            print(json.dumps({'figure': 'lookahead_cost', 'cfg': cfg, 'failed': rc}), flush=True)
            sys.exit(rc)
