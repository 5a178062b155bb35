"""tools/recipe_heuristic_cost.py - what the recipe heuristic costs and what it buys (include/ngw.h ngw_snapshot_recipe_costs /
ngw_search_set_recipe; pool.recipe_costs, search.RecipeHeuristic), one JSON line per figure.

    python tools/recipe_heuristic_cost.py [--rounds 5] [--figures call,iteration,expanded] [--parent-lib PATH]

Everything timed is timed by a HIP event pair on torch's stream (the wall clock to a final sync beside it); medians of `rounds` rounds with
minimum and maximum, microseconds.  Sizes: 4 096 and 65 536 slots, 10 x 10 and 32 x 32 Pogostick maps.

"call" (one process): P envs, ten random committed steps, saved into a pool of P slots; a device list of all P slots.
    call_us   pool.recipe_costs(slots, device=True)
    keys_us   pool.keys(slots, device=True) - the kernel that reads the same rows in the same shape
    loop_us   the loop the call replaces: pool.state(), search.recipe_cost_reference(inv, map_item_counts(map)) in numpy, the result uploaded
The three run interleaved, their order alternating between the rounds.

"iteration" (one child process per library and round, the libraries taking turns and the order alternating): one open-list iteration of
tools/best_first_cost.py's cost rows - P roots, keep = 4096, capacity = max(P, 4096), the real step costs, a table sized by a dry run, a new
search per timed run, two iterations timed and divided by two - for
    parent_none   the library given with --parent-lib (the parent commit's build), no heuristic; left out without --parent-lib
    none          this library, no heuristic: must sit inside the spread DESIGN.md 4.22 to 4.26 record for one library
    recipe        this library, RecipeHeuristic()
    recipe_walk   this library, RecipeHeuristic(WalkHeuristic(24 on the crafting table, 'min'))
    walk          this library, the walk heuristic alone (what 4.26 measured)
A child times every size once, its own forms interleaved.

"expanded" (one process): states expanded until proven() on tools/best_first_cost.py's goal scenario - the 9 x 9 goal state, two roots - under
the REAL costs at scale 1, prune, keep = 64, lists of 4096, a pool of 2^18 slots, at most 4000 iterations: h = 0, walk only, recipe, recipe + walk.
A run that ends with a flag raised or without proven() is reported as it ended."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.best_first_cost import KEEP, crafting_weights, stats  # noqa: E402

SIZES = [(P, S) for P in (4096, 65536) for S in (10, 32)]
POGO = 'NovelGridworld-Pogostick-v1'


def event_pair(fn, sync):
    """fn() between two events on torch's stream -> (event us, wall us)."""
    import torch
    sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    fn()
    t1.record()
    sync()
    return t0.elapsed_time(t1) * 1e3, (time.perf_counter() - w0) * 1e6


def call_figure(P, S, rounds):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd import search as SR
    v = VecNovelGridworld(spec=make_spec(POGO, S), num_envs=P, seed=3)
    v.reset()
    rs = np.random.RandomState(1)
    for _ in range(10):
        v.step(rs.randint(0, v.n_actions, P).astype(np.int32))
    pool = v.snapshot(P)
    pool.save(envs=np.arange(P), slots=np.arange(P))
    slots = torch.arange(P, dtype=torch.int32, device='cuda')
    program = SR.recipe_program(v.spec)

    def sync():
        torch.cuda.synchronize()
        v.sync()

    def loop():
        st = pool.state()
        h = SR.recipe_cost_reference(st['inv'], SR.map_item_counts(st['map'], v.n_items), program)
        return torch.from_numpy(h).cuda()

    forms = [('call', lambda: pool.recipe_costs(slots, device=True)), ('keys', lambda: pool.keys(slots, device=True)), ('loop', loop)]
    same = bool((forms[0][1]().cpu().numpy() == loop().cpu().numpy()).all())
    for _, fn in forms:
        fn()
    res = {name + suffix: [] for name, _ in forms for suffix in ('_us', '_wall_us')}
    for r in range(rounds):
        for name, fn in (forms if r % 2 == 0 else forms[::-1]):
            ev, wall = event_pair(fn, sync)
            res[name + '_us'].append(ev)
            res[name + '_wall_us'].append(wall)
    out = {'figure': 'recipe_call', 'slots': P, 'map_size': S, 'rounds': rounds, 'device': torch.cuda.get_device_name(0), 'call_equals_loop': same, 'flags': v.error_flags()}
    out.update({k: stats(x) for k, x in res.items()})
    out['loop_over_call'] = round(out['loop_us']['us'] / out['call_us']['us'], 1)
    out['call_over_keys'] = round(out['call_us']['us'] / out['keys_us']['us'], 2)
    pool.close()
    v.close()
    return out


def iteration_child(forms, iterations=2):
    """One round of the "iteration" figure in this process's library: {size: {form: event us per iteration}}."""
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.search import RecipeHeuristic
    out = {}
    for P, S in SIZES:
        v = VecNovelGridworld(spec=make_spec(POGO, S), num_envs=P, seed=3)
        v.reset()
        A, cap = v.n_actions, max(P, KEEP)
        pool = v.snapshot(P + iterations * KEEP * A)
        pool.save(envs=np.arange(P), slots=np.arange(P))
        roots = torch.arange(P, dtype=torch.int32, device='cuda')
        walk = crafting_weights(v, 24)
        heur = {'none': lambda: None, 'parent_none': lambda: None, 'walk': lambda: walk, 'recipe': lambda: RecipeHeuristic(), 'recipe_walk': lambda: RecipeHeuristic(walk)}

        def sync():
            torch.cuda.synchronize()
            v.sync()

        def run(s):
            s.reset_cursor(P)
            s.start(roots)
            s.run(iterations)

        probe = v.key_table(2 * (P + iterations * cap * A), values=True)
        sp = pool.search(probe, cap, keep=KEEP, open_list=True)
        run(sp)
        v.sync()
        stored = len(probe)
        sp.close(), probe.close()
        table = v.key_table(2 * stored, values=True)
        row = {}
        for timed in (False, True):                                            # a warm pass first (the selection's scratch grows there)
            for name in forms:
                table.clear()
                s = pool.search(table, cap, keep=KEEP, open_list=True, heuristic=heur[name]())
                ev, _ = event_pair(lambda: run(s), sync)
                if timed:
                    row[name] = ev / iterations
                s.close()
        v.error_flags()
        out['%dx%d' % (P, S)] = row
        table.close(), pool.close(), v.close()
    return out


def iteration_figure(rounds, parent_lib):
    mine = ['none', 'recipe', 'recipe_walk', 'walk']
    libs = [('this', None, mine)] + ([('parent', parent_lib, ['parent_none'])] if parent_lib else [])
    rows = {}
    for r in range(rounds):
        for _, lib, forms in (libs if r % 2 == 0 else libs[::-1]):
            forms = forms if r % 2 == 0 else forms[::-1]
            env = dict(os.environ)
            if lib:
                env['NGW_LIB'] = os.path.abspath(lib)
            got = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', ','.join(forms)], env=env, capture_output=True, text=True, timeout=600)
            if got.returncode:
                raise RuntimeError(got.stderr[-2000:])
            for size, row in json.loads(got.stdout.strip().splitlines()[-1]).items():
                for name, us in row.items():
                    rows.setdefault(size, {}).setdefault(name, []).append(us)
    out = []
    for (P, S) in SIZES:
        row = rows['%dx%d' % (P, S)]
        line = {'figure': 'recipe_iteration', 'roots': P, 'map_size': S, 'keep': KEEP, 'rounds': rounds, 'parent_lib': bool(parent_lib)}
        line.update({name + '_us': stats(x) for name, x in row.items()})
        for name in ('recipe', 'recipe_walk', 'walk'):
            line[name + '_minus_none_us'] = round(line[name + '_us']['us'] - line['none_us']['us'], 1)
        out.append(line)
    return out


def expanded_figure():
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.search import RecipeHeuristic
    spec = make_spec(POGO, 9)
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
    walk = crafting_weights(v, 24)
    out = {'figure': 'recipe_expanded', 'map_size': 9, 'keep': 64, 'capacity': 4096, 'pool': 1 << 18, 'costs': 'the step costs at scale 1'}
    for name, heur in (('h0', None), ('walk', walk), ('recipe', RecipeHeuristic()), ('recipe_walk', RecipeHeuristic(walk))):
        pool, table = v.snapshot(1 << 18), v.key_table(1 << 19, values=True)
        pool.save(envs=np.arange(4), slots=np.arange(4))
        s = pool.search(table, 4096, scale=1, keep=64, open_list=True, prune=True, heuristic=heur)
        s.reset_cursor(4)
        s.start(np.arange(2))
        w0, expanded = time.perf_counter(), 0
        while not s.proven() and s.stats().iterations < 4000 and not s.stats().flags:
            s.run(8)
            os_ = s.open_stats()                                                       # (the ring keeps 64 iterations: add up as they come)
            expanded += int((os_.chosen[-8:] - os_.pruned[-8:]).sum())
        out[name] = {'proven': bool(s.proven()), 'iterations': int(s.stats().iterations), 'expanded': expanded, 'goal': int(s.goal().value),
                     'slots': int(s.stats().cursor), 'flags': int(s.stats().flags), 'wall_ms': round((time.perf_counter() - w0) * 1e3, 1)}
        for x in (s, pool, table):
            x.close()
        v.error_flags()
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--figures', default='call,iteration,expanded')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(iteration_child(args.child.split(','))), flush=True)
        return
    figures = args.figures.split(',')
    if 'call' in figures:
        for P, S in SIZES:
            print(json.dumps(call_figure(P, S, args.rounds)), flush=True)
    if 'iteration' in figures:
        for line in iteration_figure(args.rounds, args.parent_lib):
            print(json.dumps(line), flush=True)
    if 'expanded' in figures:
        print(json.dumps(expanded_figure()), flush=True)


if __name__ == '__main__':
    main()
