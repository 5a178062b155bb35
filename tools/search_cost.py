"""tools/search_cost.py - what one iteration of a search run costs (include/ngw.h ngw_search_run, Search.run) beside one iteration of the
hand-written loop it replaces (key_table.py's docstring, as tests/test_search_run.py copies it), one JSON line per shape.

    python tools/search_cost.py [--rounds 5] [--iterations 2] [--rows 0,1,...,7]

One process.  A row is (parents P, map size S, keep): P envs of an S x S Pogostick map saved into the first P slots of a pool of P * (1 +
iterations) slots, a search of capacity P with the real step costs, a valued table sized from a dry run so that its load after the timed
iterations is at most 1/4.  Per round and form: the table is cleared, the roots are started, and `iterations` iterations are timed - by a HIP
event pair on torch's stream (both forms end ordered before it) and, separately, by wall clock from the first enqueue to a final sync().  The
order of the two forms alternates between the rounds.  Medians of `rounds` rounds with minimum and maximum, microseconds per iteration:
    run_us / run_wall_us     Search.run(iterations): one library call
    loop_us / loop_wall_us   the hand-written loop: nine library calls and the torch operations between them per iteration
host_calls and launches are NOT measured: they are read off the code of the two forms and written into the line as constants (`counted:
"read off the code"`) - host_calls the library calls Python makes per iteration, launches the kernels of the library per iteration (a memset
of select's grid form counted as one), torch's own kernels in the loop not counted.  The table's buckets are a power of two, so a load of
exactly 1/4 cannot be set: `load` is the one measured, between 1/8 and 1/4.  No bar is set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(P, S, keep) for P in (4096, 65536) for S in (10, 32) for keep in (None, 4096)]


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def measure(row, rounds, iterations):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.key_table import VALUE_NONE, step_cost_values
    from gym_novel_gridworlds_amd.spec import IDX_NONE
    P, S, keep = ROWS[row]
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', S), num_envs=P, seed=3)
    v.reset()
    A, cap_pool = v.n_actions, P * (1 + iterations)
    pool = v.snapshot(cap_pool)
    pool.save(envs=np.arange(P), slots=np.arange(P))
    roots = torch.arange(P, dtype=torch.int32, device='cuda')
    arange_a = torch.arange(A, dtype=torch.int32, device='cuda')
    zeros = torch.zeros(P, dtype=torch.int32, device='cuda')
    fr = pool.frontier(P)

    g = torch.full((cap_pool + 1,), VALUE_NONE, dtype=torch.int32, device='cuda')          # (made once, as the search makes its own once)
    bucket = torch.full((cap_pool + 1,), -1, dtype=torch.int32, device='cuda')

    def loop(table):
        fr.reset_cursor(P)

        def note(slots, where):
            at = torch.where(slots != IDX_NONE, slots, cap_pool).long()
            g[at], bucket[at] = table.read(where, device=True)[0], where
            g[cap_pool], bucket[cap_pool] = VALUE_NONE, -1
        parents = roots
        _, found = pool.insert_keys_min(table, parents, zeros, device=True)
        note(parents, found.where)
        for _ in range(iterations):
            succ = pool.successor_keys(parents, device=True)
            live, pi = (parents != IDX_NONE)[:, None], parents.clamp(min=0).long()
            g_child = torch.where(live, g[pi][:, None] + step_cost_values(succ.info), VALUE_NONE).to(torch.int32).contiguous()
            tags = (bucket[pi][:, None] * A + arange_a[None, :]).to(torch.int32)
            found = table.insert_min(succ.keys.reshape(-1), g_child.reshape(-1), tags=tags.reshape(-1).contiguous(), device=True)
            if keep is None:
                p, a = fr.compact(found.best, A, parents)
            else:
                sel = fr.select(g_child, keep, A, parents, flags=found.best)
                p, a = sel.first, sel.second
            c = fr.alloc()
            pool.expand(p, a, c, device=True)
            note(c, table.lookup(pool.keys(c, device=True), device=True))
            parents = c.clone()

    def run(s):
        s.reset_cursor(P)
        s.start(roots)
        s.run(iterations)

    def timed(fn, arg, table):
        """-> (event us, wall us) per iteration of one fn(arg) on a cleared table; the start of the roots is inside both forms' times."""
        table.clear()
        torch.cuda.synchronize(); v.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        fn(arg)
        t1.record()
        torch.cuda.synchronize(); v.sync()
        w1 = time.perf_counter()
        return t0.elapsed_time(t1) * 1e3 / iterations, (w1 - w0) * 1e6 / iterations

    probe = v.key_table(P * (1 + iterations * A), values=True)                 # the dry run: how many keys the timed iterations store
    loop(probe)
    stored = len(probe)
    probe.close()
    tables = [v.key_table(2 * stored, values=True) for _ in range(2)]          # buckets >= 4 * stored: a load of at most 1/4
    s = pool.search(tables[0], P, keep=keep)
    forms = [('run', run, s, tables[0]), ('loop', loop, tables[1], tables[1])]
    for _, fn, arg, table in forms:                                            # warm both
        timed(fn, arg, table)
    v.error_flags()
    res = {'run_us': [], 'run_wall_us': [], 'loop_us': [], 'loop_wall_us': []}
    for r in range(rounds):
        for name, fn, arg, table in (forms if r % 2 == 0 else forms[::-1]):
            ev, wall = timed(fn, arg, table)
            res[name + '_us'].append(ev)
            res[name + '_wall_us'].append(wall)
    st = s.stats()
    assert len(tables[0]) == len(tables[1]) == stored and st.cursor == int(fr.cursor.item())
    choose = 2 if keep is None else (1 if P * A <= 1024 else 7)
    out = {'figure': 'search_cost', 'parents': P, 'map_size': S, 'keep': keep, 'iterations': iterations, 'rounds': rounds,
           'device': torch.cuda.get_device_name(0), 'stored': stored, 'buckets': tables[0].buckets, 'load': round(stored / tables[0].buckets, 3),
           'improved': st.improved.tolist(), 'expanded': st.expanded.tolist(), 'flags': v.error_flags(),
           'counted': 'read off the code', 'host_calls': {'run': round(1 / iterations, 2), 'loop': 9},
           'launches': {'run': 8 + choose, 'loop': 8 + choose}}
    for k, x in res.items():
        out[k] = stats(x)
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=2)
    ap.add_argument('--rows', default=','.join(str(i) for i in range(len(ROWS))))
    a = ap.parse_args()
    for r in a.rows.split(','):
        measure(int(r), a.rounds, a.iterations)
