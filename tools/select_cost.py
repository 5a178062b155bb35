"""tools/select_cost.py - what a priority frontier costs (include/ngw.h ngw_frontier_select, Frontier.select) beside the torch chain it replaces, one
JSON line per shape.

    python tools/select_cost.py [--rounds 5] [--reps 20] [--rows 0,1,2,3,4,5]

One process per row: the parent opens no device and starts a fresh child for every row, which measures both forms in the same process.  A row is
(groups, m, keep) over values [groups * m] drawn from a range of 64 path costs - heavy ties at the cut -, flags at density 1/2 and a parent map with
div = A = 17:
    rows 0 .. 3   groups = 1,  n = 4 096 x 17 and 65 536 x 17,  keep = 256 and 4 096        (the grid form: a pool's whole successor table)
    rows 4, 5     groups = 4 096 and 65 536,  m = 8 x 17,  keep = 8                         (the wave form: a beam of 8 per env)
Per row, medians of `rounds` rounds with their minimum and maximum, in microseconds per call over `reps` calls inside one HIP event pair:
    select_us   Frontier.select (event pair on the env's stream)
    torch_us    masked values -> torch.topk -> sort of the chosen indices -> div / mod -> gather through the map (event pair on torch's stream); for
                groups > 1 the topk runs along dim 1 of the [groups, m] view.  The chain has no defined winner among equal values and no taken /
                bound / count outputs; it is the nearest thing a caller could write today.
No bar is set."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A = 17
ROWS = [(1, 4096 * A, 256), (1, 4096 * A, 4096), (1, 65536 * A, 256), (1, 65536 * A, 4096), (4096, 8 * A, 8), (65536, 8 * A, 8)]


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def measure(row, rounds, reps):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.key_table import VALUE_NONE
    groups, m, keep = ROWS[row]
    n = groups * m
    dev = 'cuda:0'
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', 10), num_envs=64, seed=1)
    v.reset()
    pool = v.snapshot(64)
    fr = pool.frontier(groups * keep)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    values = torch.randint(0, 64, (n,), dtype=torch.int32, device=dev, generator=g)
    flags = torch.randint(0, 2, (n,), device=dev, generator=g) == 1
    amap = torch.randperm(n // A, device=dev, generator=g).to(torch.int32)
    offsets = (torch.arange(groups, device=dev) * m)[:, None]
    torch.cuda.synchronize()

    def select():
        return fr.select(values, keep, A, amap, flags, groups)

    def chain():
        masked = torch.where(flags, values, VALUE_NONE).view(groups, m)
        idx = torch.topk(masked, keep, dim=1, largest=False, sorted=False).indices
        pos = (torch.sort(idx, dim=1).values + offsets).reshape(-1)
        q = torch.div(pos, A, rounding_mode='floor')
        return amap[q], pos - q * A

    def select_us():
        torch.cuda.synchronize(); v.sync()
        v.timing_begin()
        for _ in range(reps):
            select()
        return v.timing_end() * 1e3 / reps

    def torch_us():
        torch.cuda.synchronize(); v.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            chain()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / reps

    for fn in (select_us, torch_us):
        fn()
    res = {'select_us': [], 'torch_us': []}
    for _ in range(rounds):
        res['select_us'].append(select_us())
        res['torch_us'].append(torch_us())
    sel = select()
    v.sync()
    out = {'figure': 'select_cost', 'groups': groups, 'm': m, 'keep': keep, 'div': A, 'form': 'wave' if m <= 1024 else 'grid', 'rounds': rounds, 'reps': reps,
           'device': torch.cuda.get_device_name(0), 'candidates': fr.total(), 'taken': int(sel.taken.sum().item())}
    for k, x in res.items():
        out[k] = stats(x)
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rows', default=','.join(str(i) for i in range(len(ROWS))))
    ap.add_argument('--row', type=int, default=None, help='measure this row in this process (what the parent starts for every row)')
    a = ap.parse_args()
    if a.row is not None:
        measure(a.row, a.rounds, a.reps)
    else:
        for r in a.rows.split(','):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--row', r, '--rounds', str(a.rounds), '--reps', str(a.reps)])
