"""tools/best_first_cost.py - what the open list costs and what the walk heuristic buys (include/ngw.h ngw_search_create_open,
pool.search(open_list=True)), one JSON line per row.

    python tools/best_first_cost.py [--rounds 5] [--iterations 2] [--rows 0,1,...,8]

One process, one library.

Rows 0 to 7, "cost": (roots P, map size S, heuristic).  P envs of an S x S Pogostick map saved into the first P slots of a pool of
P + iterations * 4096 * A slots; keep = 4096, capacity = max(P, 4096) for both forms; the real step costs; a valued table sized from a dry
run to a load of at most 1/4.  Per round and form: the table is cleared, the roots are started, and `iterations` iterations are timed by a
HIP event pair on torch's stream (and by wall clock to a final sync).  The forms run interleaved and their order alternates between the
rounds; every round makes a new search of each form on its cleared table, outside the timed region (an open list is not restarted: its f, h
and slot_of_bucket would be the last round's).  Medians of `rounds` rounds with minimum and maximum, microseconds per iteration:
    beam_us   Search.run with keep=4096 (the beam: the 4096 cheapest children of the iteration go on)
    open_us   Search.run with open_list=True, keep=4096 - and, in the heuristic rows, WalkHeuristic(24 on the crafting table, 'min')
The open form adds a selection over the whole pool and, with a heuristic, a walk over `capacity` children, so it is expected to cost more;
the difference is reported as it comes out.  The two forms do not do the same work after the first iteration - the beam drops what the
open list keeps - so `expanded` of both is part of the line.  No bar is set.

Row 8, "expanded": the states expanded (sum of chosen - pruned) until proven(), h = 0 against the walk heuristic, on one fixed scenario with
a reachable goal: the 9 x 9 Pogostick map of tests/test_search_run.py's goal_state - the agent at (3, 3) facing east, a crafting table at
(4, 4), the sticks, planks and rubber of a pogo stick in the inventory, so the goal is two moves and a craft away -, two roots, per-action
costs Left 1, Right 10, every other action 5 (the goal costs 12), keep = 4, prune, a pool of 512 and lists of 256; the heuristic is weight
1 (the cheapest move) on the crafting table, 'min'.  Both searches run until proven() with no state lost (flags 0)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEP = 4096
ROWS = [(P, S, heur) for P in (4096, 65536) for S in (10, 32) for heur in (False, True)]


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def crafting_weights(v, weight):
    from gym_novel_gridworlds_amd.search import WalkHeuristic
    w = np.zeros(v.n_items, np.int32)
    w[v.spec.items_id['crafting_table']] = weight
    return WalkHeuristic(w, 'min')


def measure(row, rounds, iterations):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    P, S, heur = ROWS[row]
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', S), num_envs=P, seed=3)
    v.reset()
    A, cap = v.n_actions, max(P, KEEP)
    cap_pool = P + iterations * KEEP * A
    pool = v.snapshot(cap_pool)
    pool.save(envs=np.arange(P), slots=np.arange(P))
    roots = torch.arange(P, dtype=torch.int32, device='cuda')

    def run(s):
        s.reset_cursor(P)
        s.start(roots)
        s.run(iterations)

    def timed(make, table):
        """-> (event us, wall us) per iteration, and the search: a NEW search on the cleared table - an open list is not restarted (its f, h and
        slot_of_bucket would be the last round's) -, made and destroyed outside the timed region."""
        table.clear()
        s = make(table)
        torch.cuda.synchronize(); v.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        run(s)
        t1.record()
        torch.cuda.synchronize(); v.sync()
        w1 = time.perf_counter()
        return t0.elapsed_time(t1) * 1e3 / iterations, (w1 - w0) * 1e6 / iterations, s

    probe = v.key_table(2 * (P + iterations * cap * A), values=True)           # the dry run: how many keys the timed iterations store at most
    sp = pool.search(probe, cap, keep=KEEP, open_list=True)
    run(sp)
    v.sync()
    stored = len(probe)
    sp.close(), probe.close()
    tables = [v.key_table(2 * stored, values=True) for _ in range(2)]
    weights = crafting_weights(v, 24) if heur else None
    forms = [('beam', lambda t: pool.search(t, cap, keep=KEEP), tables[0]),
             ('open', lambda t: pool.search(t, cap, keep=KEEP, open_list=True, heuristic=weights), tables[1])]
    for _, make, table in forms:                                               # warm both (the selection's scratch grows here, not in a timed round)
        timed(make, table)[2].close()
    v.error_flags()
    res = {'beam_us': [], 'beam_wall_us': [], 'open_us': [], 'open_wall_us': []}
    last = {}
    for r in range(rounds):
        for name, make, table in (forms if r % 2 == 0 else forms[::-1]):
            ev, wall, s = timed(make, table)
            res[name + '_us'].append(ev)
            res[name + '_wall_us'].append(wall)
            if name in last:
                last[name].close()
            last[name] = s
    beam, open_ = last['beam'], last['open']
    out = {'figure': 'best_first_cost', 'roots': P, 'map_size': S, 'keep': KEEP, 'capacity': cap, 'pool': cap_pool, 'heuristic': heur, 'iterations': iterations,
           'rounds': rounds, 'device': torch.cuda.get_device_name(0), 'buckets': tables[0].buckets,
           'beam_expanded': beam.stats().expanded[-iterations:].tolist(), 'open_expanded': open_.stats().expanded[-iterations:].tolist(),
           'open_chosen': open_.open_stats().chosen[-iterations:].tolist(), 'open_superseded': open_.open_stats().superseded[-iterations:].tolist(),
           'flags': v.error_flags()}
    for k, x in res.items():
        out[k] = stats(x)
    out['open_over_beam'] = round(out['open_us']['us'] / out['beam_us']['us'], 2)
    for x in (beam, open_, tables[0], tables[1], pool):
        x.close()
    v.close()
    return out


def expanded_until_proven():
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.spec import ACT_LEFT, ACT_RIGHT
    spec = make_spec('NovelGridworld-Pogostick-v1', 9)
    v = VecNovelGridworld(spec=spec, num_envs=4, seed=4)
    v.reset()
    S, ids, st = v.map_size, spec.items_id, v.get_state()
    m = st['map'].reshape(v.num_envs, S, S)
    m[:, 3, 3] = m[:, 3, 4] = m[:, 4, 3] = 0
    m[:, 4, 4] = ids['crafting_table']
    st['loc'][:], st['facing'][:], st['inv'][:] = [3, 3], 3, 0
    for name, q in (('stick', 4), ('plank', 2), ('rubber', 1)):
        st['inv'][:, ids[name]] = q
    v.set_state(0, map=st['map'], loc=st['loc'], facing=st['facing'], inv=st['inv'], selected=st['selected'], step_count=st['step_count'])
    cs = spec.compile()
    kinds = [int(cs.act_kind[a]) for a in range(cs.n_actions)]
    costs = np.full(cs.n_actions, 5, np.int32)
    costs[kinds.index(ACT_LEFT)], costs[kinds.index(ACT_RIGHT)] = 1, 10
    out = {'figure': 'best_first_expanded', 'map_size': 9, 'keep': 4, 'costs': 'Left 1, Right 10, else 5'}
    for name, heur in (('h0', None), ('walk', crafting_weights(v, 1))):
        pool, table = v.snapshot(512), v.key_table(2048, values=True)
        pool.save(envs=np.arange(4), slots=np.arange(4))
        s = pool.search(table, 256, costs=costs, keep=4, open_list=True, prune=True, heuristic=heur)
        s.reset_cursor(4)
        s.start(np.arange(2))
        while not s.proven() and s.stats().iterations < 200:
            s.run(2)
        os_ = s.open_stats()
        out[name] = {'proven': bool(s.proven()), 'iterations': int(os_.iterations), 'expanded': int((os_.chosen - os_.pruned).sum()), 'goal': int(s.goal().value),
                     'slots': int(s.stats().cursor), 'flags': int(s.stats().flags)}
        for x in (s, pool, table):
            x.close()
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=2)
    ap.add_argument('--rows', default=','.join(str(i) for i in range(len(ROWS) + 1)))
    args = ap.parse_args()
    for row in (int(x) for x in args.rows.split(',')):
        print(json.dumps(expanded_until_proven() if row == len(ROWS) else measure(row, args.rounds, args.iterations)), flush=True)


if __name__ == '__main__':
    main()
