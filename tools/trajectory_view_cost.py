"""tools/trajectory_view_cost.py - what recording AgentMap views costs a playout / a slot rollout (include/ngw.h ngw_snapshot_playout_traj_views /
_rollout_traj_views), one JSON line per call, map size, pair count and path length.

    python tools/trajectory_view_cost.py [--pairs 4096,65536] [--cfgs C2,S32] [--steps 8,64] [--calls playout,rollout] [--view 5] [--reps 3] [--rounds 5]

tools/trajectory_cost.py with the views in the place of the lidar rows: ONE process runs every shape, each shape after the other; the first one
that fails ends the run.  `n` pairs whose parents are `n` random slots of one snapshot of 4 096 saved states (they repeat), autoreset off, nothing
kept, no lidar configured - all device tensors, allocated once per shape outside the timed windows.  After a warm-up, `rounds` rounds alternate the
variants; every figure is a HIP event pair on the env's stream around a window of `reps` repetitions (the average INCLUDING the gaps between
launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    path       the path call of the same shape without keys (ngw_snapshot_playout_path / _rollout_path with every pointer NULL)
    views      the trajectory call with the three view buffers [T + 1, n, ...] and nothing else          -> (a) views / path = what the recording costs
    step_loop  the loop the call replaces: T times a one-step rollout(children=scratch) + agent_view(scratch) on the recorded actions, the rows
               ping-ponging between the two halves of a scratch pool of 2 n rows                        -> (b) step_loop / views
The loop's three fields are checked against the call's (equal, block for block) before anything is timed.  `scratch_MiB` is the memory the loop's
scratch pool takes and the call does not; `obs_MiB` is what the three buffers take.  No bar: the comparison is between the variants on the same
build.  As in trajectory_cost.py the call is timed through the C-ABI on preallocated buffers and the loop through the Python wrappers a caller would
write it with, so (b) is what a caller's loop pays, host work included - not a ratio of device work."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}
NODES = 4096
FIELDS = ('agent_map', 'agent_facing_id', 'inventory_items_quantity')


def shape(args, call, cfg, n, T):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A, V = len(spec.actions_id), args.view
    W = 2 * V + 1
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, NODES), dtype=torch.int32, device=dev, generator=g)
    parents = torch.randint(0, NODES, (n,), dtype=torch.int32, device=dev, generator=g)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)   # noqa: E731
    ret, length, ended, info, first = i32(n), i32(n), torch.zeros(n, dtype=torch.uint8, device=dev), i32(n), i32(n)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=NODES, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    nodes, scratch = v.snapshot(), v.snapshot(2 * n)
    nodes.save()
    v.sync()
    K, pad = v.n_items, (n + 63) // 64 * 64
    view = torch.zeros((T + 1, pad, W, W), dtype=torch.int8, device=dev)
    facing, inv = i32(T + 1, pad), i32(T + 1, pad, K)
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    vw = _cabi.TrajViews(V, view.data_ptr(), facing.data_ptr(), inv.data_ptr(), pad)
    half = [torch.arange(0, n, dtype=torch.int32, device=dev), torch.arange(n, 2 * n, dtype=torch.int32, device=dev)]
    # the actions every variant of this shape runs: the playout's own record, or random plans
    if call == 'playout':
        actions = nodes.playout(parents, T, 12345, record=True, device=True).actions.clamp(min=0)   # (-1 behind an end: never executed again)
    else:
        actions = torch.randint(0, A, (T, n), dtype=torch.int32, device=dev, generator=g)
    torch.cuda.synchronize()
    rep = (ptr(ret), ptr(length), ptr(ended), ptr(info))
    out = {}

    def views():
        if call == 'playout':
            _cabi.check(L.ngw_snapshot_playout_traj_views(v._h, nodes._s, ptr(parents), n, T, 12345, 0, None, None, None, None, *rep, ptr(first), None, 0, 0, None, 0,
                                                          None, 0, None, 0, None, 0, C.byref(vw)))
        else:
            _cabi.check(L.ngw_snapshot_rollout_traj_views(v._h, nodes._s, ptr(parents), ptr(actions), n, T, None, None, None, n, *rep, 0, None, 0, None, 0, None, 0,
                                                          C.byref(vw)))

    def path():
        if call == 'playout':
            _cabi.check(L.ngw_snapshot_playout_path(v._h, nodes._s, ptr(parents), n, T, 12345, 0, None, None, None, None, *rep, ptr(first), None, 0, 0, None, 0))
        else:
            _cabi.check(L.ngw_snapshot_rollout_path(v._h, nodes._s, ptr(parents), ptr(actions), n, T, None, None, None, n, *rep, 0, None, 0))

    def step_loop():
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        rows = [nodes.agent_view(parents, view_size=V, device=True)]
        for t in range(T):
            src, idx = (nodes, parents) if t == 0 else (scratch, half[t % 2])
            e = scratch.rollout(idx, actions[t:t + 1], half[(t + 1) % 2], source=src, device=True)
            o = scratch.agent_view(half[(t + 1) % 2], view_size=V, device=True)
            rows.append({k: torch.where(alive.reshape((n,) + (1,) * (x.dim() - 1)), x, torch.zeros_like(x)) for k, x in o.items()})
            alive &= ~e.ended
        for k in FIELDS:
            out[k] = torch.stack([r[k] for r in rows])

    variants = {'path': path, 'views': views, 'step_loop': step_loop}
    res = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    v.sync()
    torch.cuda.synchronize()
    for k, mine in zip(FIELDS, (view, facing, inv)):
        assert torch.equal(out[k], mine[:, :n]), (call, cfg, n, T, 'the loop and the call disagree on ' + k)
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
    row_bytes = S * S + 4 * (K + 1) + 8 + 4 + 1 + 4 + 4
    obs_row = W * W + 4 + 4 * K
    line = {'figure': 'trajectory_view_cost', 'call': call, 'cfg': cfg, 'S': S, 'view_size': V, 'pairs': n, 'T': T, 'reps': args.reps, 'rounds': args.rounds,
            'device': torch.cuda.get_device_name(0), 'scratch_MiB': round(2 * n * row_bytes / 2 ** 20, 1), 'obs_row_bytes': obs_row,
            'obs_MiB': round((T + 1) * pad * obs_row / 2 ** 20, 1), 'executed_steps': int(length.sum())}
    for k, x in res.items():
        line[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    line['views_over_path'] = round(line['views']['us'] / line['path']['us'], 2)
    line['step_loop_over_views'] = round(line['step_loop']['us'] / line['views']['us'], 2)
    print(json.dumps(line), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', default='4096,65536')
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--steps', default='8,64')
    ap.add_argument('--calls', default='playout,rollout')
    ap.add_argument('--view', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for call in a.calls.split(','):
        for cfg in a.cfgs.split(','):
            for n in a.pairs.split(','):
                for t in a.steps.split(','):
                    shape(a, call, cfg, int(n), int(t))
