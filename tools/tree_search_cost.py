"""tools/tree_search_cost.py - what one iteration of a tree-search run costs (include/ngw.h ngw_tree_run, TreeSearch.run) beside one iteration of
the hand-written loop it replaces (README "Guided playouts": a guided playout, table.insert of the leaves, playout.tree_steps, two index_add_
calls and the rows recomputed in torch), one JSON line per shape.

    python tools/tree_search_cost.py [--rounds 5] [--iterations 4] [--rows 0,1,...,8]

One process.  A row is (roots P, map size S, steps T, same): P envs of an S x S Pogostick map saved into a pool, a tree of P playouts of T steps
with c = 2; `same`: every root is slot 0 - the contention case, where every lane of every wave backs up into one (bucket, action) at t = 0.  The
loop is given the mask words for free from the playout's recorded `masks`, and its sums are int32 / int64 index_add_ calls, so that it computes
the same rows: before anything is timed, both forms run `iterations` iterations and their statistics are compared THROUGH THE KEYS - the
roots' keys and every leaf key the loop offered to its table: both tables hold exactly those, and visits, returns, mask words and rows at
table.lookup of each are equal - a difference ends the row.  Per round and form: the table and the statistics are
cleared, the roots started, and `iterations` iterations timed - by a HIP event pair on torch's stream (both forms end ordered before it) and,
separately, by wall clock from the first enqueue to a final sync().  The order of the two forms alternates between the rounds.  Medians of
`rounds` rounds with minimum and maximum, microseconds per iteration:
    run_us / run_wall_us     TreeSearch.run(iterations): one library call
    loop_us / loop_wall_us   the hand-written loop: two library calls and the torch operations between them per iteration
In the contention row also the backup stage alone (TreeSearch.backup over one recorded playout; event pair, per call): backup_us with the
in-wave combining, backup_plain_us on a second tree made with plain_backup=True.  No bar is set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(P, S, T, False) for P in (4096, 65536) for S in (10, 32) for T in (8, 64)] + [(65536, 10, 8, True)]
C_PUCT = 2.0


def stats(x):
    return {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}


def measure(row, rounds, iterations):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, make_spec
    from gym_novel_gridworlds_amd.playout import tree_steps
    P, S, T, same = ROWS[row]
    v = VecNovelGridworld(spec=make_spec('NovelGridworld-Pogostick-v1', S), num_envs=P, seed=3)
    v.reset()
    A = v.n_actions
    pool = v.snapshot(P)
    pool.save()
    roots = torch.zeros(P, dtype=torch.int32, device='cuda') if same else torch.arange(P, dtype=torch.int32, device='cuda')
    cap = 4 * P * (1 + iterations)                                     # (load at most 1/8 after the timed iterations)
    table, table2 = v.key_table(cap), v.key_table(cap)
    t = pool.tree_search(table, P, T, c=C_PUCT)
    B = table2.buckets
    N, Q = torch.zeros((B, A), dtype=torch.int32, device='cuda'), torch.zeros((B, A), dtype=torch.int64, device='cuda')
    M, W = torch.zeros(B, dtype=torch.int64, device='cuda'), torch.zeros((B, A), dtype=torch.float32, device='cuda')
    arange_a, steps, j = torch.arange(A, device='cuda'), torch.arange(T, device='cuda')[:, None], torch.arange(P, device='cuda')
    c = torch.tensor(C_PUCT, dtype=torch.float32, device='cuda')

    def rows_of(b):
        """the PUCT rows of buckets b in torch: float32, one operation at a time (torch does not contract eager operations)"""
        n, m = N[b], M[b]
        q = torch.where(n > 0, Q[b].float() / n.clamp(min=1).float(), torch.zeros((), device='cuda'))
        u = (c * 1.0) * torch.sqrt((n.long().sum(1) + 1).float())[:, None] / (1 + n).float()
        valid = ((m[:, None] >> arange_a) & 1).bool()
        score = torch.where(valid, q + u, torch.full((), -float('inf'), device='cuda'))
        best = score.max(1, keepdim=True).values
        first = ((score == best) & valid).int().argmax(1)
        W[b] = torch.nn.functional.one_hot(first, A).float() * valid.any(1, keepdim=True)

    def loop_start():
        table2.clear()
        for x in (N, Q, M, W):
            x.zero_()
        w0 = table2.insert(pool.keys(roots, device=True), device=True).where.long()
        M[w0] = pool.sample_actions(roots, torch.zeros((A, P), dtype=torch.float32, device='cuda'), 0, device=True).mask_words
        rows_of(torch.unique(w0))

    offered = []

    def loop_iteration(i):
        r = pool.playout(roots, T, 7, first_pair=i * P, record=True, path_keys=True, rewards=True, masks=True, table=table2, table_weights=W, device=True)
        d, n = r.depth.long(), r.length.long()
        has = (d >= 1) & (d < n)
        dc = d.clamp(0, T - 1)
        leaf = torch.where(has, r.keys[(d - 1).clamp(0, T - 1), j], torch.zeros_like(r.keys[0]))
        offered.append(leaf)
        wl = table2.insert(leaf, device=True).where
        ok = wl >= 0
        M[wl.long()[ok]] = r.masks[dc, j][ok]
        where = r.where.clone()
        where[dc[ok], j[ok]] = wl[ok]
        where[(steps > d[None, :]) | (d[None, :] < 1)] = -1
        G = torch.flip(torch.cumsum(torch.flip(r.rewards.long(), [0]), 0), [0])
        b, a, tt, jj = tree_steps(r._replace(where=where))
        N.view(-1).index_add_(0, b * A + a, torch.ones_like(b, dtype=torch.int32))
        Q.view(-1).index_add_(0, b * A + a, G[tt, jj])
        rows_of(torch.unique(b))

    def run_form():
        t.clear()
        t.start(roots)
        return lambda: t.run(iterations, 7)

    def loop_form():
        loop_start()

        def go():
            for i in range(iterations):
                loop_iteration(i)
        return go

    # equality first, through the keys
    run_form()()
    loop_form()()
    v.sync()
    keys = torch.unique(torch.cat([pool.keys(roots, device=True)] + offered))
    keys = keys[keys != 0]
    offered.clear()
    b1, b2 = table.lookup(keys, device=True).long(), table2.lookup(keys, device=True).long()
    same_stats = bool((b1 >= 0).all() and (b2 >= 0).all() and len(table) == len(table2) == int(keys.numel()) and (t.visits[b1] == N[b2]).all() and
                      (t.returns[b1] == Q[b2]).all() and (t.mask_words[b1] == M[b2]).all() and (t.rows[b1] == W[b2]).all())
    if not same_stats:
        raise SystemExit("row %d: the run and the hand-written loop differ" % row)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {'run': ([], []), 'loop': ([], [])}
    for k in range(rounds):
        for name in (('run', 'loop') if k % 2 == 0 else ('loop', 'run')):
            go = run_form() if name == 'run' else loop_form()
            torch.cuda.synchronize()
            v.sync()
            t0 = time.perf_counter()
            ev[0].record()
            go()
            offered.clear()
            v.stream_order(torch.cuda.current_stream().cuda_stream, False)
            ev[1].record()
            torch.cuda.synchronize()
            v.sync()
            out[name][1].append((time.perf_counter() - t0) * 1e6 / iterations)
            out[name][0].append(ev[0].elapsed_time(ev[1]) * 1e3 / iterations)
    line = dict(row=row, roots=P, map=S, steps=T, same_root=same, iterations=iterations, rounds=rounds, keys=len(table), equal=same_stats,
                run_us=stats(out['run'][0]), run_wall_us=stats(out['run'][1]), loop_us=stats(out['loop'][0]), loop_wall_us=stats(out['loop'][1]))
    if same:
        r = pool.playout(roots, T, 7, first_pair=99 * P, record=True, path_keys=True, rewards=True, masks=True, table=table, table_weights=t.rows, device=True)
        plain = pool.tree_search(table, P, T, c=C_PUCT, plain_backup=True)
        for name, x in (('backup_us', t), ('backup_plain_us', plain)):
            x.backup(r)
            times = []
            for _ in range(rounds):
                torch.cuda.synchronize()
                v.sync()
                ev[0].record()
                x.backup(r)
                ev[1].record()
                torch.cuda.synchronize()
                times.append(ev[0].elapsed_time(ev[1]) * 1e3)
            line[name] = stats(times)
    v.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=4)
    ap.add_argument('--rows', default=','.join(str(i) for i in range(len(ROWS))))
    a = ap.parse_args()
    for row in [int(x) for x in a.rows.split(',')]:
        print(json.dumps(measure(row, a.rounds, a.iterations)), flush=True)


if __name__ == '__main__':
    main()
