"""tools/tree_rule_cost.py - what the rule of ngw_tree_set_rule costs and buys (include/ngw.h; TreeSearch spread=, discount=), one JSON line per figure.

    python tools/tree_rule_cost.py [--rounds 5] [--iterations 4] [--parts forms,spread,default,buys]

One process per library.  Shapes are tools/tree_search_cost.py's: P envs of an S x S Pogostick map saved into a pool, a tree of P playouts of T steps,
c = 2, a table at a load below 1/8.  HIP event pairs on torch's stream, medians of `rounds` rounds with [min, max]; the order of the forms alternates
between the rounds.
    forms    the reweight stage alone at spread 1 (t.reweight() over the `touched` list of a real iteration, T * P entries): the one-lane kernel
             (rows16=2) against the 16-lane kernel (rows16=1) on the same statistics; the rows' bytes are compared first.  P in {4096, 65536}, T in {8, 64}.
    spread   the reweight stage and a whole iteration at spread 1, 8 and 64.
    default  a default tree's whole iteration, for comparing this library with the parent's: run the tool once as it is and once with
             NGW_LIB=<the parent's library> (--parts default); the lines carry the library's path.
    buys     nodes grown per iteration and the largest depth at spread 1, 8, 64: 64 roots in one state (64 playouts per root state), 16 iterations,
             from t.stats().
No bar is set."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_PUCT = 2.0
SHAPES = [(P, 10, T) for P in (4096, 65536) for T in (8, 64)]


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def setup(P, S, T, iterations, same=False, **kw):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', S), num_envs=max(P, 4), seed=3)
    v.reset()
    pool = v.snapshot(max(P, 4))
    pool.save()
    roots = torch.zeros(P, dtype=torch.int32, device='cuda') if same else torch.arange(P, dtype=torch.int32, device='cuda')
    table = v.key_table(4 * P * (1 + iterations) * max(1, min(kw.get('spread', 1), 8)))
    return v, pool, table, roots


def timed(v, calls, rounds, per=1):
    """calls: name -> a function that enqueues the work on the env's stream -> name -> stats in microseconds per `per`."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in calls}
    names = list(calls)
    for k in range(rounds):
        for name in (names if k % 2 == 0 else names[::-1]):
            prepare, go = calls[name]
            prepare()
            torch.cuda.synchronize()
            v.sync()
            ev[0].record()
            go()
            v.stream_order(torch.cuda.current_stream().cuda_stream, False)
            ev[1].record()
            torch.cuda.synchronize()
            v.sync()
            out[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / per)
    return {k: stats(x) for k, x in out.items()}


def forms(rounds, iterations):
    import torch
    for P, S, T in SHAPES:
        v, pool, table, roots = setup(P, S, T, iterations)
        trees = {name: pool.tree_search(table, P, T, c=C_PUCT, rows16=r) for name, r in (('one_lane', 2), ('rows16', 1))}
        t = trees['one_lane']
        t.start(roots)
        t.run(iterations, 7)                                              # real statistics and a real `touched` list
        other = trees['rows16']
        for name in ('visits', 'returns', 'mask_words'):
            getattr(other, name).copy_(getattr(t, name))
        touched = t.last['touched'].reshape(-1).clone()
        for x in trees.values():
            x.rows.zero_()
            x.reweight(touched)
        equal = bool((t.rows.view(torch.int32) == other.rows.view(torch.int32)).all()) and bool(t.rows.any())
        if not equal:
            raise SystemExit("forms %s: the two kernels' rows differ" % ((P, S, T),))
        res = timed(v, {name: ((lambda: None), (lambda x=x: x.reweight(touched))) for name, x in trees.items()}, rounds)
        print(json.dumps(dict(part='forms', roots=P, map=S, steps=T, entries=int(touched.numel()), listed=int((touched >= 0).sum()), equal=equal, **res)), flush=True)
        v.close()


def spread_cost(rounds, iterations):
    for P, S, T in SHAPES:
        for spread in (1, 8, 64):
            v, pool, table, roots = setup(P, S, T, iterations, spread=spread)
            t = pool.tree_search(table, P, T, c=C_PUCT, spread=spread)
            t.start(roots)
            t.run(iterations, 7)
            touched = t.last['touched'].reshape(-1).clone()

            def again():
                t.clear()
                t.start(roots)
            res = timed(v, {'reweight': ((lambda: None), (lambda: t.reweight(touched)))}, rounds)
            res.update(timed(v, {'iteration': (again, (lambda: t.run(iterations, 7)))}, rounds, iterations))
            print(json.dumps(dict(part='spread', roots=P, map=S, steps=T, spread=spread, keys=len(table), **res)), flush=True)
            v.close()


def default(rounds, iterations):
    from gym_novel_gridworlds_amd import _cabi
    for P, S, T in ((4096, 10, 8), (65536, 10, 64)):
        v, pool, table, roots = setup(P, S, T, iterations)
        t = pool.tree_search(table, P, T, c=C_PUCT)

        def again():
            t.clear()
            t.start(roots)
        again()
        t.run(iterations, 7)
        res = timed(v, {'iteration': (again, (lambda: t.run(iterations, 7)))}, rounds, iterations)
        print(json.dumps(dict(part='default', library=_cabi.LIB_PATH, roots=P, map=S, steps=T, keys=len(table), **res)), flush=True)
        v.close()


def buys(iterations=16):
    for spread in (1, 8, 64):
        v, pool, table, roots = setup(64, 10, 12, iterations, same=True, spread=8)
        t = pool.tree_search(table, 64, 12, c=C_PUCT, spread=spread)
        t.start(roots)
        t.run(iterations, 7)
        st = t.stats()
        print(json.dumps(dict(part='buys', spread=spread, playouts=64, steps=12, iterations=iterations, grown=st.grown.tolist(), depth=st.depth.tolist(),
                              nodes=len(table), flags=st.flags)), flush=True)
        v.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=4)
    ap.add_argument('--parts', default='forms,spread,default,buys')
    a = ap.parse_args()
    for part in a.parts.split(','):
        if part == 'buys':
            buys()
        else:
            {'forms': forms, 'spread': spread_cost, 'default': default}[part](a.rounds, a.iterations)


if __name__ == '__main__':
    main()
