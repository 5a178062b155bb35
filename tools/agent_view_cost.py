"""tools/agent_view_cost.py - what keeping the AgentMap window current costs per batched step (include/ngw.h ngw_agent_view_fuse), one JSON line
per shape.

    python tools/agent_view_cost.py [--counts 4096,65536] [--sizes 10,20,32] [--views 5,2] [--cfgs plain,fire] [--reps 200] [--rounds 5]

One process.  Device-resident int32 actions, autoreset with horizon 100 (prepared next episodes at the library's default), a warm-up of 40 steps.
The variants run one after the other, each behind an untimed window of its own, `rounds` rounds back to back; every figure is a HIP event pair on the env's stream around a window of `reps` steps (the average
INCLUDING the gaps between launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum, in us per
step:
    step        (a) step_device alone, the switch off
    two_launch  (b) step_device + ngw_agent_view: the two launches a caller issues without the switch
    fused       (c) set_agent_view(V): the step kernel's VIEW form where the launch has one
    gather      (d) set_agent_view(V, fused=False): the library enqueues the gather behind every step
NGW_VIEW_FUSE=16 makes (c) the step kernel's form at every view_size (the library fuses view_size <= 2 by default).  (c) and (d) are skipped on a library without the entry point (NGW_LIB=<an older build>: the same tool measures (a) and (b) of the parent commit).
After the timing the tool asserts that (b), (c) and (d), run from the same state with the same actions, leave the same windows.  plain:
Pogostick-v1; fire: Pogostick-v1 + FireWall (the EXT kernels).  No bar is set here: DESIGN.md 4.20 holds the table and the rule."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape(args, cfg, S, n, V, out):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    from gym_novel_gridworlds_amd.novelty import apply_novelty
    spec = make_spec('NovelGridworld-Pogostick-v1', S)
    if cfg == 'fire':
        apply_novelty(spec, 'firewall', 'medium', '', '')
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    acts = torch.randint(0, A, (args.reps, n), dtype=torch.int32, device=dev, generator=g)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1, autoreset=True, horizon=100)
    L = _cabi.lib()
    has = hasattr(L, 'ngw_agent_view_fuse') and not args.ab_only
    v.reset()
    for t in range(40):
        v.step_device(acts[t % args.reps].data_ptr())
    v.sync()
    snap = v.snapshot()
    snap.save()
    ptrs = [acts[t].data_ptr() for t in range(args.reps)]
    step = L.ngw_step_device
    view = L.ngw_agent_view
    h = v._h

    def run_step():
        for p in ptrs:
            step(h, p)

    def run_two():
        for p in ptrs:
            step(h, p)
            view(h, V)
    variants = [('step', 0, run_step), ('two_launch', 0, run_two)]
    if has:
        variants += [('fused', 1, run_step), ('gather', 2, run_step)]
    res = {k: [] for k, _, _ in variants}
    windows = {}
    for k, on, fn in variants:                                # (the windows each variant leaves from the saved state)
        if has:
            _cabi.check(L.ngw_agent_view_fuse(h, V, on))
        snap.restore(keep_episode=False)
        fn()
        if k != 'step':
            windows[k] = v.agent_view(V, device=True).clone()
    for k, on, fn in variants:
        # variant by variant: the switch synchronises the stream, and a window that starts on a drained stream reads up to 3 us per step high
        # at 4 096 envs - so it is thrown once per variant, a whole untimed window runs behind it, and the rounds follow back to back
        if has:
            _cabi.check(L.ngw_agent_view_fuse(h, V, on))
        fn()
        for r in range(args.rounds):
            v.timing_begin()
            fn()
            res[k].append(v.timing_end() * 1e3 / args.reps)
    v.sync()
    for k in windows:
        assert bool((windows[k] == windows['two_launch']).all()), (cfg, S, n, V, k)
    assert v.error_flags() == 0
    W = 2 * V + 1
    row = {'figure': 'agent_view_cost', 'cfg': cfg, 'S': S, 'n': n, 'V': V, 'view_B_per_env': W * W, 'reps': args.reps, 'rounds': args.rounds,
           'lib': os.path.basename(os.path.dirname(os.path.abspath(_cabi.LIB_PATH))) + '/' + os.path.basename(_cabi.LIB_PATH), 'device': torch.cuda.get_device_name(0)}
    for k, x in res.items():
        row[k] = {'us': round(float(np.median(x)), 2), 'min': round(float(min(x)), 2), 'max': round(float(max(x)), 2)}
    print(json.dumps(row), flush=True)
    if out:
        out.write(json.dumps(row) + '\n')
        out.flush()
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--sizes', default='10,20,32')
    ap.add_argument('--views', default='5,2')
    ap.add_argument('--cfgs', default='plain,fire')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ab-only', action='store_true', help='(a) and (b) only, the entry point never called: how an older library is measured')
    ap.add_argument('--out', default='', help='also append the JSON lines to this file')
    a = ap.parse_args()
    out = open(a.out, 'a') if a.out else None
    for cfg in a.cfgs.split(','):
        for S in a.sizes.split(','):
            for n in a.counts.split(','):
                for V in a.views.split(','):
                    shape(a, cfg, int(S), int(n), int(V), out)
