"""tools/frontier_cost.py - what device-side frontiers cost and save (include/ngw.h ngw_frontier_compact / ngw_frontier_alloc, NGW_IDX_NONE), one JSON
line per map size and parent count.

    python tools/frontier_cost.py [--counts 4096,65536] [--rounds 5] [--reps 10] [--cfgs C2,S32]

One process.  Per configuration (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32) and count: a handle of `count` envs after 20 random steps, a
pool whose first `count` slots hold their states (the parents) with room for count * A children behind them, and a key table for all of them.
Medians of `rounds` rounds, each figure with its minimum and maximum, in microseconds:
  (a) compact_us / nonzero_us    Frontier.compact of a [count, A] flag array at density 1/17 (capacity count * A) against torch.nonzero + floor
                                 division + remainder on the same flags; both in wall time per call over `reps` calls with one synchronisation at
                                 the end of the window (torch.nonzero waits for the host inside every call).
  (b) bfs_frontier / bfs_host    one breadth-first iteration - table.clear, insert_successor_keys, the pairs, the slots, expand - in the new form at
                                 capacity count * A, and the same iteration through snapshot.fresh_pairs and host-chosen slots (the dense form):
                                 `event_us` a HIP event pair on the env's stream around the iteration, `wall_us` perf_counter around it with
                                 a device synchronisation at its end.
  (c) expand_padded / expand_dense   ngw_snapshot_expand of count * A pairs of which the first 1/17 are live and the others NGW_IDX_NONE (what the
                                 early exit leaves of a padded launch) against the expand of the live pairs alone; event pairs over `reps` calls.
No bar is set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def measure(cfg, n, rounds, reps):
    import torch
    from gym_novel_gridworlds_amd import IDX_NONE, VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.snapshot import fresh_pairs
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    cap = n * A
    pool = v.snapshot(n + cap)
    pool.save(slots=np.arange(n))
    table = v.key_table(2 * cap)
    parents = torch.arange(n, dtype=torch.int32, device=dev)
    fr = pool.frontier(cap)
    v.sync()
    out = {'figure': 'frontier_cost', 'cfg': cfg, 'n': n, 'S': S, 'A': A, 'capacity': cap, 'rounds': rounds, 'reps': reps,
           'device': torch.cuda.get_device_name(0)}

    # ---- (a) compaction against nonzero + div / mod
    flags = (torch.randint(0, 17, (n, A), device=dev, generator=g) == 0)
    torch.cuda.synchronize()

    def by_nonzero():
        pos = torch.nonzero(flags.reshape(-1)).reshape(-1)
        return torch.div(pos, A, rounding_mode='floor'), pos % A

    def wall(fn, k):
        torch.cuda.synchronize(); v.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize(); v.sync()
        return (time.perf_counter() - t0) * 1e6 / k
    for fn in (lambda: fr.compact(flags, A), by_nonzero):
        wall(fn, 2)
    res = {'compact_us': [], 'nonzero_us': []}
    for _ in range(rounds):
        res['compact_us'].append(wall(lambda: fr.compact(flags, A), reps))
        res['nonzero_us'].append(wall(by_nonzero, reps))
    for k, x in res.items():
        out[k] = stats(x)
    out['hits'] = fr.total()

    # ---- (b) one breadth-first iteration, both forms
    def it_frontier():
        table.clear()
        fr.reset_cursor(n)
        succ, found = pool.insert_successor_keys(table, parents, device=True)
        p, a = fr.fresh_pairs(found.fresh, parents)
        c = fr.alloc()
        pool.expand(p, a, c, device=True)

    def it_host():
        table.clear()
        succ, found = pool.insert_successor_keys(table, parents, device=True)
        p, a = fresh_pairs(found.fresh)
        k = int(p.numel())
        children = torch.arange(n, n + k, dtype=torch.int32, device=dev)
        pool.expand(parents[p].contiguous(), a.to(torch.int32).contiguous(), children, device=True)

    for name, fn in (('bfs_frontier', it_frontier), ('bfs_host', it_host)):
        fn(); fn()
        torch.cuda.synchronize(); v.sync()
    ev = {'bfs_frontier': [], 'bfs_host': []}
    wl = {'bfs_frontier': [], 'bfs_host': []}
    for _ in range(rounds):
        for name, fn in (('bfs_frontier', it_frontier), ('bfs_host', it_host)):
            torch.cuda.synchronize(); v.sync()
            v.timing_begin()
            fn()
            ev[name].append(v.timing_end() * 1e3)
            wl[name].append(wall(fn, 1))
    for name in ev:
        out[name] = {'event_us': stats(ev[name]), 'wall_us': stats(wl[name])}
    out['fresh_children'] = fr.total()

    # ---- (c) a padded expand against the dense one
    live = cap // 17
    acts = torch.randint(0, A, (cap,), dtype=torch.int32, device=dev, generator=g)
    none = torch.full((cap - live,), IDX_NONE, dtype=torch.int32, device=dev)
    p_pad = torch.cat([torch.randint(0, n, (live,), dtype=torch.int32, device=dev, generator=g), none]).contiguous()
    c_pad = torch.cat([torch.arange(n, n + live, dtype=torch.int32, device=dev), none]).contiguous()
    p_dense, c_dense, a_dense = p_pad[:live].contiguous(), c_pad[:live].contiguous(), acts[:live].contiguous()
    torch.cuda.synchronize()
    forms = {'expand_padded': lambda: pool.expand(p_pad, acts, c_pad, device=True), 'expand_dense': lambda: pool.expand(p_dense, a_dense, c_dense, device=True)}
    res = {k: [] for k in forms}
    for fn in forms.values():
        fn(); fn()
    v.sync()
    for _ in range(rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize(); v.sync()
            v.timing_begin()
            for _ in range(reps):
                fn()
            res[k].append(v.timing_end() * 1e3 / reps)
    for k, x in res.items():
        out[k] = stats(x)
    out['live_pairs'] = live
    assert v.error_flags() == 0
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cfgs', default='C2,S32')
    a = ap.parse_args()
    for cfg in a.cfgs.split(','):
        for n in a.counts.split(','):
            measure(cfg, int(n), a.rounds, a.reps)
