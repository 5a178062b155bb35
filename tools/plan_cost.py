"""tools/plan_cost.py - what scoring P candidate plans of T steps costs (include/ngw.h ngw_plan_eval), one JSON line per shape.

    python tools/plan_cost.py [--n 65536] [--reps 20] [--rounds 5] [--cfgs C2,C3,C5]

One child process per configuration (C2 Pogostick-v1 10 x 10, C3 Bow-v1 20 x 20, C5 AddItem 32 x 32), each under its own time limit; the
first one that fails ends the run.  Per configuration the shapes P in {4, 16} x T in {8, 32}, autoreset off so that every variant does the
same work.  Every variant runs on a FRESH handle (same seed, same warm-up steps: the same state); after a warm-up, `rounds` rounds alternate
the variants; every figure is a HIP event pair on the env's stream around a window of repetitions (the average INCLUDING the gaps between
launches - what a caller's loop pays):
    plan_eval           ngw_plan_eval, blocks ordered env-block-major (the default)
    plan_eval_pm        the same kernel with the blocks ordered plan-major (NGW_PLAN_ORDER=plan when the handle first evaluates)
    snapshot_loop       what a user runs without it: snapshot.save() once, then per plan restore(keep_episode=True) + rollout_actions with
                        reward / done rows + a torch reduction of the rows to ret / length / ended (and info where the plan ran to its last
                        step: the rows do not carry the info word of an earlier step), all on one stream
The tool asserts that plan_eval, plan_eval_pm and snapshot_loop agree.  The bar: plan_eval beats snapshot_loop by more than the spread
(max - min) of either side, at every shape."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10, None), 'C3': ('NovelGridworld-Bow-v1', 20, None),
       'C5': ('NovelGridworld-Pogostick-v1', 32, ('additem', 'hard', 'arrow', ''))}
SHAPES = [(4, 8), (4, 32), (16, 8), (16, 32)]


def make(cfg, n, acts):
    from gym_novel_gridworlds_amd import VecNovelGridworld, apply_novelty, make_spec
    env_id, S, nov = CFG[cfg]
    spec = make_spec(env_id, S)
    if nov:
        apply_novelty(spec, *nov)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    for t in range(acts.shape[0]):                            # the same few steps on every handle: the variants start from one state
        v.step_device(acts[t].data_ptr())
    v.sync()
    return v


def child(args):
    import torch
    from gym_novel_gridworlds_amd import _cabi, make_spec, apply_novelty
    cfg, n = args.child, args.n
    env_id, S, nov = CFG[cfg]
    spec = make_spec(env_id, S)
    if nov:
        apply_novelty(spec, *nov)
    A = len(spec.actions_id)
    g = torch.Generator(device='cuda:0')
    g.manual_seed(7)
    acts = torch.randint(0, A, (20, n), dtype=torch.int32, device='cuda:0', generator=g)
    for P, T in SHAPES:
        plans = torch.randint(0, A, (T, P, n), dtype=torch.int32, device='cuda:0', generator=g)
        torch.cuda.synchronize()
        # ---- the three variants, a fresh handle each
        os.environ.pop('NGW_PLAN_ORDER', None)
        va = make(cfg, n, acts)
        va.evaluate_plans_ptr(plans.data_ptr(), n, P, T)      # (the first evaluation reads the block order)
        os.environ['NGW_PLAN_ORDER'] = 'plan'
        vc = make(cfg, n, acts)
        vc.evaluate_plans_ptr(plans.data_ptr(), n, P, T)
        os.environ.pop('NGW_PLAN_ORDER', None)
        vb = make(cfg, n, acts)
        ts = torch.cuda.Stream()                              # the loop's env and its torch reductions share ONE stream
        vb.set_stream(ts.cuda_stream)
        snap = vb.snapshot()
        snap.save()
        rows_r = torch.zeros((T, n), dtype=torch.int32, device='cuda:0')
        rows_d = torch.zeros((T, n), dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        vb.rollout_outputs(rows_r.data_ptr(), rows_d.data_ptr(), n, False)
        out3 = vb.device_outputs()
        loop = {'ret': torch.zeros((P, n), dtype=torch.int32, device='cuda:0'), 'length': torch.zeros((P, n), dtype=torch.int32, device='cuda:0'),
                'ended': torch.zeros((P, n), dtype=torch.bool, device='cuda:0'), 'info': torch.zeros((P, n), dtype=torch.int32, device='cuda:0')}

        def snapshot_loop():
            for p in range(P):
                snap.restore(keep_episode=True)
                vb.rollout_actions(plans[0, p].data_ptr(), P * n, T)
                with torch.cuda.stream(ts):
                    d = rows_d != 0
                    alive = (torch.cumsum(d, 0) - d.int()) == 0           # no step before this one ended the episode
                    loop['ret'][p] = (rows_r * alive).sum(0)
                    loop['length'][p] = alive.sum(0)
                    loop['ended'][p] = (d & alive).any(0)
                    loop['info'][p] = out3['info']
        variants = {'plan_eval': (lambda: va.evaluate_plans_ptr(plans.data_ptr(), n, P, T), va, args.reps),
                    'plan_eval_pm': (lambda: vc.evaluate_plans_ptr(plans.data_ptr(), n, P, T), vc, args.reps),
                    'snapshot_loop': (snapshot_loop, vb, max(2, args.reps // 5))}
        res = {k: [] for k in variants}
        for k, (fn, v, reps) in variants.items():
            for _ in range(2):
                fn()
            v.sync()
        for r in range(args.rounds):
            for k, (fn, v, reps) in variants.items():
                v.timing_begin()
                for _ in range(reps):
                    fn()
                res[k].append(v.timing_end() * 1e3 / reps)
        # ---- the three answers agree
        ea = va.evaluate_plans(plans, device=True)
        ec = vc.evaluate_plans(plans, device=True)
        snapshot_loop()
        torch.cuda.synchronize()
        for k in ('ret', 'length', 'ended', 'info'):
            assert bool((ea[k] == ec[k]).all()), (cfg, P, T, k, 'block orders')
        for k in ('ret', 'length', 'ended'):
            assert bool((ea[k].t() == loop[k]).all()), (cfg, P, T, k, 'snapshot loop')
        full = ea['length'].t() == T
        assert bool((ea['info'].t()[full] == loop['info'][full]).all()), (cfg, P, T, 'info')
        assert va.error_flags() == 0 and vb.error_flags() == 0 and vc.error_flags() == 0
        out = {'figure': 'plan_cost', 'cfg': cfg, 'n': n, 'S': S, 'P': P, 'T': T, 'reps': args.reps, 'rounds': args.rounds,
               'mean_length': round(float(ea['length'].float().mean()), 2)}
        for k, x in res.items():
            out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
        pe, lo = out['plan_eval'], out['snapshot_loop']
        spread = max(pe['max'] - pe['min'], lo['max'] - lo['min'])
        out['loop_over_plan_eval'] = round(lo['us'] / pe['us'], 1)
        out['plan_major_over_env_block_major'] = round(out['plan_eval_pm']['us'] / pe['us'], 3)
        out['bar_plan_eval_beats_the_loop_by_more_than_the_spread'] = bool(lo['us'] - pe['us'] > spread)
        print(json.dumps(out), flush=True)
        snap = None
        va.close(); vb.close(); vc.close()
        if not out['bar_plan_eval_beats_the_loop_by_more_than_the_spread']:
            sys.exit(3)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,C3,C5')
    ap.add_argument('--limit', type=int, default=240, help='seconds per configuration')
    ap.add_argument('--child', default='')
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', str(a.n),
                              '--reps', str(a.reps), '--rounds', str(a.rounds)])
        if rc:
            print(json.dumps({'figure': 'plan_cost', 'cfg': cfg, 'failed': rc}), flush=True)
            sys.exit(rc)
