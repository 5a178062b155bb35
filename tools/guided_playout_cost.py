"""tools/guided_playout_cost.py - what a guided playout (Snapshot.playout(table=, table_weights=); include/ngw.h ngw_snapshot_playout_guided) costs
against the host loop it replaces and against the weighted path-form playout, one JSON line per shape.

    python tools/guided_playout_cost.py [--pairs 4096,65536] [--cfgs C2,S32] [--steps 8,64] [--loads 0.25,0.5] [--hits 0,0.5,1] [--reps 3] [--rounds 5]

ONE process runs every shape, each after the other; the first one that fails ends the run.  `n` pairs whose parents are `n` random slots of one
snapshot of 4 096 saved states (they repeat), autoreset off, nothing kept.  The table: every row of table_weights equals the default weight vector,
so the guided playout visits exactly the states of the weighted playout (the bit identity of the contract - asserted before anything is timed) and
the states it will look up are known beforehand.  A share `hit` of those states' distinct keys (chosen by a bit of the key) is inserted, then random
filler keys until the table holds load * buckets keys; buckets is the smallest power of two that holds all visited keys at a load of 1/4, so the probe
chains are the load's and the row reads go to a tensor of buckets * A floats.  `hit_rate` is the measured share of executed steps with where >= 0.
After a warm-up, `rounds` rounds alternate the variants; every figure is a HIP event pair on the env's stream around a window of `reps` repetitions
(the average INCLUDING the gaps between launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    weighted   playout(weights=w, path_keys=True): the weighted path-form playout                      -> guided / weighted = the price of the guidance
    guided     playout(weights=w, path_keys=True, table=, table_weights=)
    loop       the loop the call replaces, T times: keys -> table.lookup -> gather the rows (torch) -> sample_actions -> a one-step
               rollout(children=scratch), the rows ping-ponging between the halves of a scratch pool of 2 n rows   -> loop / guided
All three go through the Python wrappers with device=True, so host work is included in all of them.  The loop draws under the sampling call's own
stream, not the playout's, so its actions are not the call's bit for bit (the distribution is); it keeps stepping pairs whose episode has ended (a
caller would mask them: one more torch op).  No bar: the comparison is between the variants on the same build."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}
NODES = 4096
SEED = 12345


def shape(args, cfg, n, T, load, hit):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, NODES), dtype=torch.int32, device=dev, generator=g)
    parents = torch.randint(0, NODES, (n,), dtype=torch.int32, device=dev, generator=g)
    w = torch.tensor([1.0 + (a % 3) for a in range(A)], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=NODES, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    nodes, scratch = v.snapshot(), v.snapshot(2 * n)
    nodes.save()
    v.sync()
    half = [torch.arange(0, n, dtype=torch.int32, device=dev), torch.arange(n, 2 * n, dtype=torch.int32, device=dev)]
    # the states the guided playout will look up: the parents and what every step but the last leaves, on the weighted playout's path
    ref = nodes.playout(parents, T, SEED, weights=w, path_keys=True, device=True)
    looked = torch.cat([nodes.keys(parents, device=True), ref.keys[:T - 1].reshape(-1)])
    visited = torch.unique(looked[looked != 0])
    capacity = 1 << max(int(2 * visited.numel() - 1).bit_length(), 4)           # buckets = 2 * capacity >= 4 * visited: a load of 1/4 holds them all
    table = v.key_table(capacity)
    target = int(load * table.buckets)
    chosen = visited if hit >= 1 else (visited[:0] if hit <= 0 else visited[((visited >> 17) & 1) == 1])
    if chosen.numel():
        table.insert(chosen.contiguous(), device=True)
    filler = torch.randint(1, 1 << 62, (max(target - int(chosen.numel()), 0),), dtype=torch.int64, device=dev, generator=g) | (1 << 62)
    if filler.numel():
        table.insert(filler, device=True)
    stored = len(table)
    tw = w.expand(table.buckets, A).contiguous()
    torch.cuda.synchronize()
    out = {}

    def weighted():
        out['weighted'] = nodes.playout(parents, T, SEED, weights=w, path_keys=True, device=True)

    def guided():
        out['guided'] = nodes.playout(parents, T, SEED, weights=w, path_keys=True, table=table, table_weights=tw, device=True)

    def loop():
        for t in range(T):
            src, idx = (nodes, parents) if t == 0 else (scratch, half[t % 2])
            keys = src.keys(idx, device=True)
            where = table.lookup(keys, device=True)
            rows = torch.where((where >= 0)[:, None], tw[where.clamp(min=0).long()], w[None, :])
            s = src.sample_actions(idx, rows.t().contiguous(), SEED, t=t, device=True)
            out['loop'] = scratch.rollout(idx, s.action.reshape(1, n), half[(t + 1) % 2], source=src, device=True)

    variants = {'weighted': weighted, 'guided': guided, 'loop': loop}
    res = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    v.sync()
    torch.cuda.synchronize()
    gd, wt = out['guided'], out['weighted']
    for name in ('ret', 'length', 'first_action', 'keys'):
        assert torch.equal(gd[name], wt[name]), (cfg, n, T, load, hit, 'equal rows: the guided and the weighted playout disagree on ' + name)
    executed = int(gd.length.sum())
    hits = int((gd.where >= 0).sum())
    out.clear()
    for r in range(args.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            v.timing_begin()
            for _ in range(args.reps):
                fn()
            v.stream_order(torch.cuda.current_stream(0).cuda_stream, True)    # the window closes behind torch's share of the loop
            res[k].append(v.timing_end() * 1e3 / args.reps)
            out.clear()
    v.sync()
    torch.cuda.synchronize()
    assert v.error_flags() == 0
    line = {'figure': 'guided_playout_cost', 'cfg': cfg, 'S': S, 'pairs': n, 'T': T, 'load': round(stored / table.buckets, 3), 'buckets': table.buckets,
            'hit_asked': hit, 'hit_rate': round(hits / max(executed, 1), 3), 'executed_steps': executed, 'reps': args.reps, 'rounds': args.rounds,
            'device': torch.cuda.get_device_name(0), 'rows_MiB': round(table.buckets * A * 4 / 2 ** 20, 1)}
    for k, x in res.items():
        line[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    line['guided_over_weighted'] = round(line['guided']['us'] / line['weighted']['us'], 2)
    line['loop_over_guided'] = round(line['loop']['us'] / line['guided']['us'], 2)
    print(json.dumps(line), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', default='4096,65536')
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--steps', default='8,64')
    ap.add_argument('--loads', default='0.25,0.5')
    ap.add_argument('--hits', default='0,0.5,1')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for cfg in a.cfgs.split(','):
        for n in a.pairs.split(','):
            for t in a.steps.split(','):
                for load in a.loads.split(','):
                    for hit in a.hits.split(','):
                        shape(a, cfg, int(n), int(t), float(load), float(hit))
