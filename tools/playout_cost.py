"""tools/playout_cost.py - what valid-action random playouts from saved states cost (include/ngw.h ngw_snapshot_playout) against the loop they
replace, one JSON line per map size, pair count and playout length.

    python tools/playout_cost.py [--pairs 4096,65536] [--cfgs C2,S32] [--steps 8,64] [--reps 3] [--rounds 5]

ONE process runs every shape, each shape after the other; the first one that fails ends the run.  `n` pairs whose parents are `n` random slots
of one snapshot of 4 096 saved states (they repeat), autoreset off, nothing kept - all device tensors.  After a warm-up, `rounds` rounds
alternate the two variants; every figure is a HIP event pair on the env's stream around a window of `reps` repetitions (the average
INCLUDING the gaps between launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    playout     ngw_snapshot_playout: one launch for all T steps
    step_loop   the loop it replaces, per step: snapshot.action_masks(nodes) -> a uniform draw among the valid actions in torch (every action
                where none is valid) -> a one-step ngw_snapshot_rollout from the scratch pool into its other half -> the reports accumulated in
                torch (pairs that ended are masked out, not compacted: no host wait inside the loop)
The two draw from different generators, so they are not compared pair by pair; the tool asserts what must hold for both: every length in
[1, T], and the same share of ended pairs within a tolerance (autoreset is off and no goal is reachable in T random steps on these maps, so
both are 0).  No bar: the comparison is between the two on the same build."""
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


def shape(args, cfg, n, T):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, NODES), dtype=torch.int32, device=dev, generator=g)
    parents = torch.randint(0, NODES, (n,), dtype=torch.int32, device=dev, generator=g)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)   # noqa: E731
    ret_a, len_a, end_a, info_a, first_a = i32(n), i32(n), torch.zeros(n, dtype=torch.uint8, device=dev), i32(n), i32(n)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=NODES, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    nodes, scratch = v.snapshot(), v.snapshot(2 * n)
    nodes.save()
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    half = [torch.arange(0, n, dtype=torch.int32, device=dev), torch.arange(n, 2 * n, dtype=torch.int32, device=dev)]
    out = {}

    def playout():
        _cabi.check(L.ngw_snapshot_playout(v._h, nodes._s, ptr(parents), n, T, 12345, 0, None, None, ptr(ret_a), ptr(len_a), ptr(end_a), ptr(info_a),
                                           ptr(first_a), None, 0))

    def step_loop():
        ret, length, alive = i32(n), i32(n), torch.ones(n, dtype=torch.bool, device=dev)
        for t in range(T):
            src, idx = (nodes, parents) if t == 0 else (scratch, half[t % 2])
            ok = src.action_masks(idx, device=True)
            ok = torch.where(ok.any(1, keepdim=True), ok, torch.ones_like(ok))
            acts = torch.multinomial(ok.float(), 1, generator=g).to(torch.int32).reshape(1, n)
            e = scratch.rollout(idx, acts, half[(t + 1) % 2], source=src, device=True)
            ret += torch.where(alive, e.ret, torch.zeros_like(e.ret))
            length += alive.to(torch.int32)
            alive &= ~e.ended
        out['b'] = (ret, length, ~alive)

    variants = {'playout': playout, 'step_loop': step_loop}
    res = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    v.sync()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            v.timing_begin()
            for _ in range(args.reps):
                fn()
            v.stream_order(torch.cuda.current_stream(0).cuda_stream, True)    # the window closes behind torch's share of the loop
            res[k].append(v.timing_end() * 1e3 / args.reps)
    v.sync()
    torch.cuda.synchronize()
    ret_b, len_b, end_b = out['b']
    assert bool(((len_a >= 1) & (len_a <= T)).all()) and bool(((len_b >= 1) & (len_b <= T)).all()), (cfg, n, T, 'lengths')
    ended = float(end_a.float().mean()), float(end_b.float().mean())
    assert abs(ended[0] - ended[1]) < 0.02, (cfg, n, T, ended)
    assert v.error_flags() == 0
    line = {'figure': 'playout_cost', 'cfg': cfg, 'S': S, 'pairs': n, 'T': T, 'reps': args.reps, 'rounds': args.rounds,
            'device': torch.cuda.get_device_name(0), 'mean_ret': [round(float(ret_a.float().mean()), 3), round(float(ret_b.float().mean()), 3)]}
    for k, x in res.items():
        line[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    line['step_loop_over_playout'] = round(line['step_loop']['us'] / line['playout']['us'], 2)
    print(json.dumps(line), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', default='4096,65536')
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--steps', default='8,64')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for cfg in a.cfgs.split(','):
        for n in a.pairs.split(','):
            for t in a.steps.split(','):
                shape(a, cfg, int(n), int(t))
