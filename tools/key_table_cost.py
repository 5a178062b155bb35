"""tools/key_table_cost.py - what the device-side key table costs (include/ngw.h ngw_key_table_insert), one JSON line per batch size and load.

    python tools/key_table_cost.py [--counts 4096,65536] [--loads 0.25,0.5] [--reps 5] [--rounds 5]

One child process per (count, load), each under its own time limit; the first one that fails ends the run.  A table of capacity 4 * count
(8 * count buckets) is filled to `load` of its BUCKETS with random keys; a batch of `count` keys, half of them already in the table and
half new, is then offered.  Every figure is a HIP event pair on the env's stream around ONE call (the table and the history are put back to
their filled state before the next one, outside the pair), reported as the median over reps * rounds calls with their minimum and maximum:
    insert          table.insert(batch, device=True): two launches
    lookup          table.lookup(batch, device=True): one launch
    unique          baseline (a): torch.unique(batch, return_inverse=True) on the batch alone - less work, it has no history
    sorted_history  baseline (b), the loop insert replaces: a sorted history tensor as large as the table's content; searchsorted for
                    membership, unique on the batch, first positions by scatter-amin, merge of the new keys and re-sort
The baselines run on torch's current stream, which is the env's stream for the run (ngw_set_stream), so that one event pair times both.
The tool checks insert's `fresh` against baseline (b)'s answer for the same batch.  No bar is set."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    n, load = args.n, args.load
    dev = 'cuda:0'
    spec = make_spec('NovelGridworld-Pogostick-v1', 10)
    v = VecNovelGridworld(spec=spec, num_envs=64, seed=1)
    v.reset()
    stream = torch.cuda.Stream(device=0)
    _cabi.check(_cabi.lib().ngw_set_stream(v._h, stream.cuda_stream))      # one stream for the table calls and the torch baselines
    table = v.key_table(4 * n)
    n_hist = int(table.buckets * load)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    with torch.cuda.stream(stream):
        pool = torch.randint(1, 1 << 62, (n_hist + n,), dtype=torch.int64, device=dev, generator=g).unique()
        pool = pool[torch.randperm(pool.numel(), device=dev, generator=g)]
        assert pool.numel() >= n_hist + n // 2
        history = pool[:n_hist].contiguous()
        batch = torch.cat([history[torch.randperm(n_hist, device=dev, generator=g)[:n - n // 2]], pool[n_hist:n_hist + n // 2]])
        batch = batch[torch.randperm(n, device=dev, generator=g)].contiguous()
        hist_sorted = history.sort().values
        stream.synchronize()

        def refill():
            table.clear()
            table.insert(history, device=True)

        def sorted_history():
            uniq, inverse = torch.unique(batch, return_inverse=True)
            at = torch.searchsorted(hist_sorted, uniq).clamp_(max=hist_sorted.numel() - 1)
            new = hist_sorted[at] != uniq
            first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=dev)
            first.scatter_reduce_(0, inverse, torch.arange(n, dtype=torch.int64, device=dev), 'amin')
            fresh = torch.zeros(n, dtype=torch.bool, device=dev)
            fresh[first[new]] = True
            merged = torch.cat([hist_sorted, uniq[new]]).sort().values
            return fresh, merged
        variants = {'insert': (lambda: table.insert(batch, device=True), refill),
                    'lookup': (lambda: table.lookup(batch, device=True), None),
                    'unique': (lambda: torch.unique(batch, return_inverse=True), None),
                    'sorted_history': (sorted_history, None)}
        refill()
        fresh_ref, merged = sorted_history()
        got = table.insert(batch, device=True)
        assert bool((got.fresh == fresh_ref).all()) and int(got.fresh.sum()) == n // 2 and len(table) == merged.numel() == n_hist + n // 2
        refill()
        for fn, _ in variants.values():                      # warm-up (allocator, kernels)
            fn()
        res = {k: [] for k in variants}
        for r in range(args.rounds):
            for k, (fn, restore) in variants.items():
                for _ in range(args.reps):
                    if restore:
                        restore()
                    v.timing_begin()
                    fn()
                    res[k].append(v.timing_end() * 1e3)
        v.sync()
    out = {'figure': 'key_table_cost', 'n': n, 'load': load, 'buckets': table.buckets, 'stored': n_hist, 'reps': args.reps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0)}
    for k, x in res.items():
        out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    out['insert_over_unique'] = round(out['insert']['us'] / out['unique']['us'], 2)
    out['insert_over_sorted_history'] = round(out['insert']['us'] / out['sorted_history']['us'], 2)
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--loads', default='0.25,0.5')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=120, help='seconds per child')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--load', type=float, default=0.25)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for n in a.counts.split(','):                             # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        for load in a.loads.split(','):
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', '--n', n, '--load', load,
                                  '--reps', str(a.reps), '--rounds', str(a.rounds)])
            if rc:
                print(json.dumps({'figure': 'key_table_cost', 'n': int(n), 'load': float(load), 'failed': rc}), flush=True)
                sys.exit(rc)
