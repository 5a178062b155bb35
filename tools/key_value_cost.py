"""tools/key_value_cost.py - what the valued key table costs (include/ngw.h ngw_key_table_insert_min / _trace), one JSON line per batch
size and load, and one per batch size and chain length.

    python tools/key_value_cost.py [--counts 4096,65536] [--loads 0.25,0.5] [--chains 8,64] [--reps 5] [--rounds 5]

One child process per line, each under its own time limit; the first one that fails ends the run.  As tools/key_table_cost.py: a table of
capacity 4 * count (8 * count buckets) is filled to `load` of its BUCKETS with random keys - here with random values in [1000, 2000) -; a
batch of `count` keys, half of them already stored and half new, with values in [0, 3000) (so some of the stored keys improve, some do not)
and one tag each, is then offered.  Every figure is a HIP event pair on the env's stream around ONE call (the table is put back to its
filled state before the next one, outside the pair), the median over reps * rounds calls with their minimum and maximum:
    insert_min   table.insert_min(batch, values, tags, device=True) on a valued table: two launches
    insert       table.insert(batch, device=True) on a table WITHOUT values, the same batch and fill: two launches
    torch_chain  what insert_min replaces: insert on the plain table, then on caller-held arrays of `buckets` entries a gather of the values
                 before, scatter_reduce(amin) of the values, a compare, a fill and scatter_reduce(amin) of the positions among the
                 candidates, a compare, and a masked store of the tags
    trace        table.trace(where, L, device=True) of `count` chains of L links each (--chains), in a table that holds count * (L + 1) keys
The torch chain runs on torch's current stream, which is the env's stream for the run (ngw_set_stream), so that one event pair times both.
The tool checks insert_min's `best`, values and tags against the chain's for the same batch, and trace's plans against the actions it wrote.
No bar is set."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(v, variants, reps, rounds):
    for fn, restore in variants.values():                    # warm-up (allocator, kernels)
        if restore:
            restore()
        fn()
    res = {k: [] for k in variants}
    for r in range(rounds):
        for k, (fn, restore) in variants.items():
            for _ in range(reps):
                if restore:
                    restore()
                v.timing_begin()
                fn()
                res[k].append(v.timing_end() * 1e3)
    v.sync()
    return {k: {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)} for k, x in res.items()}


def setup():
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', 10), num_envs=64, seed=1)
    v.reset()
    stream = torch.cuda.Stream(device=0)
    _cabi.check(_cabi.lib().ngw_set_stream(v._h, stream.cuda_stream))      # one stream for the table calls and the torch chain
    g = torch.Generator(device='cuda:0')
    g.manual_seed(11)
    return torch, v, stream, g


def child_insert(args):
    torch, v, stream, g = setup()
    from gym_novel_gridworlds_amd.key_table import TAG_ROOT, VALUE_NONE
    n, load, dev = args.n, args.load, 'cuda:0'
    valued, plain = v.key_table(4 * n, values=True), v.key_table(4 * n)
    B = valued.buckets
    n_hist = int(B * load)
    with torch.cuda.stream(stream):
        pool = torch.randint(1, 1 << 62, (n_hist + n,), dtype=torch.int64, device=dev, generator=g).unique()
        pool = pool[torch.randperm(pool.numel(), device=dev, generator=g)]
        assert pool.numel() >= n_hist + n // 2
        history = pool[:n_hist].contiguous()
        hist_values = torch.randint(1000, 2000, (n_hist,), dtype=torch.int32, device=dev, generator=g)
        batch = torch.cat([history[torch.randperm(n_hist, device=dev, generator=g)[:n - n // 2]], pool[n_hist:n_hist + n // 2]])
        batch = batch[torch.randperm(n, device=dev, generator=g)].contiguous()
        values = torch.randint(0, 3000, (n,), dtype=torch.int32, device=dev, generator=g)
        tags = torch.arange(n, dtype=torch.int32, device=dev)
        position = torch.arange(n, dtype=torch.int32, device=dev)
        # the caller-held arrays of the torch chain, one more entry for the stores that are masked out
        val, tag, first = (torch.empty(B + 1, dtype=torch.int32, device=dev) for _ in range(3))
        stream.synchronize()

        def refill_valued():
            valued.clear()
            valued.insert_min(history, hist_values, device=True)

        def refill_plain():
            plain.clear()
            plain.insert(history, device=True)

        def refill_chain():                                   # (which bucket a key gets may differ from fill to fill: the values follow `where`)
            plain.clear()
            where = plain.insert(history, device=True).where.long()
            val.fill_(VALUE_NONE)
            val[where] = hist_values
            tag.fill_(TAG_ROOT)

        def torch_chain():
            found = plain.insert(batch, device=True)
            w = torch.where(found.where >= 0, found.where, B).long()
            before = val[w]
            val.scatter_reduce_(0, w, values, 'amin')
            cand = (values == val[w]) & (values < before)
            first.fill_(n)
            first.scatter_reduce_(0, w, torch.where(cand, position, n), 'amin')
            best = cand & (first[w] == position)
            tag.scatter_(0, torch.where(best, w, B), tags)
            return found, best
        # the check of insert_min against the chain
        refill_chain()
        refill_valued()
        found, best = torch_chain()
        got = valued.insert_min(batch, values, tags, device=True)
        assert bool((got.best == best).all()) and bool((got.fresh == found.fresh).all()) and 0 < int(best.sum()) < n
        gv, gt = valued.read(got.where, device=True)
        assert bool((gv == val[found.where.long()]).all()) and bool((gt == tag[found.where.long()]).all())
        out = timed(v, {'insert_min': (lambda: valued.insert_min(batch, values, tags, device=True), refill_valued),
                        'insert': (lambda: plain.insert(batch, device=True), refill_plain),
                        'torch_chain': (torch_chain, refill_chain)}, args.reps, args.rounds)
    out.update(figure='key_value_cost', n=n, load=load, buckets=B, stored=n_hist, improved=int(best.sum()), reps=args.reps, rounds=args.rounds,
               device=torch.cuda.get_device_name(0))
    out['insert_min_over_insert'] = round(out['insert_min']['us'] / out['insert']['us'], 2)
    out['insert_min_over_torch_chain'] = round(out['insert_min']['us'] / out['torch_chain']['us'], 2)
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


def child_trace(args):
    torch, v, stream, g = setup()
    from gym_novel_gridworlds_amd.key_table import VALUE_NONE
    n, L, A, dev = args.n, args.chain, v.n_actions, 'cuda:0'
    table = v.key_table(n * (L + 1), values=True)
    with torch.cuda.stream(stream):
        keys = torch.randint(1, 1 << 62, (2 * n * (L + 1),), dtype=torch.int64, device=dev, generator=g).unique()
        keys = keys[torch.randperm(keys.numel(), device=dev, generator=g)][:n * (L + 1)].contiguous()
        assert keys.numel() == n * (L + 1)
        where = table.insert(keys, device=True).where.reshape(L + 1, n)                  # level l of chain j: where[l, j]; level 0 the roots
        acts = (torch.arange(L + 1, dtype=torch.int32, device=dev)[:, None] + torch.arange(n, dtype=torch.int32, device=dev)[None, :]) % A
        tags = torch.zeros((L + 1, n), dtype=torch.int32, device=dev)
        tags[1:] = where[:-1] * A + acts[1:]
        values = torch.zeros((L + 1, n), dtype=torch.int32, device=dev)
        values[0] = VALUE_NONE                                                         # no offer: the roots keep TAG_ROOT
        table.insert_min(keys, values.reshape(-1), tags.reshape(-1), device=True)
        ends = where[L].contiguous()
        tr = table.trace(ends, L, device=True)
        assert bool((tr.length == L).all()) and bool((tr.root == where[0]).all()) and bool((tr.plans == acts[1:]).all())
        out = timed(v, {'trace': (lambda: table.trace(ends, L, device=True), None)}, args.reps, args.rounds)
    out.update(figure='key_value_trace_cost', n=n, chain=L, buckets=table.buckets, reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--loads', default='0.25,0.5')
    ap.add_argument('--chains', default='8,64')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=120, help='seconds per child')
    ap.add_argument('--child', choices=['insert', 'trace'])
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--load', type=float, default=0.25)
    ap.add_argument('--chain', type=int, default=8)
    a = ap.parse_args()
    if a.child:
        (child_insert if a.child == 'insert' else child_trace)(a)
        sys.exit(0)
    jobs = [('insert', n, ['--load', load]) for n in a.counts.split(',') for load in a.loads.split(',')]
    jobs += [('trace', n, ['--chain', L]) for n in a.counts.split(',') for L in a.chains.split(',')]
    for kind, n, extra in jobs:                               # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', kind, '--n', n,
                              '--reps', str(a.reps), '--rounds', str(a.rounds)] + extra)
        if rc:
            print(json.dumps({'figure': 'key_value_cost', 'child': kind, 'n': int(n), 'args': extra, 'failed': rc}), flush=True)
            sys.exit(rc)
