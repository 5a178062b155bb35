"""tools/mask_cost.py - what the action masks cost (include/ngw.h ngw_set_action_mask), one JSON line per figure.

    python tools/mask_cost.py batched [--n 65536] [--steps 200] [--rounds 5]
        per batched step (device actions, eager launches) at C2 (Pogostick-v1 10 x 10), C3 (Bow-v1 20 x 20), C5 (AddItem 32 x 32), three forms
        alternated round by round: masks off / fused (the step kernel computes them) / the step followed by the standalone mask kernel
    python tools/mask_cost.py host [--n 65536] [--steps 100]
        host-API step() alone and followed by action_mask_words() (C2)
    python tools/mask_cost.py adapter [--steps 3000]
        the single-env adapter's steps/s with and without action_masks() before every step (the reference's loop shape)
    python tools/mask_cost.py lean [--steps 200]
        masks off: the step with the bit-row lidar at C2 / C3 and two EXT fused rollouts, for the library NGW_LIB names (before / after)
    python tools/mask_cost.py c2 [--steps 400]
        masks-off C2 step time of whatever library NGW_LIB names (before / after builds, alternated by the caller in fresh processes)
Wall-clock per step over `steps` steps after a warm-up, stream synchronised at both ends; median over rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10, None), 'C3': ('NovelGridworld-Bow-v1', 20, None),
       'C5': ('NovelGridworld-Pogostick-v1', 32, ('additem', 'hard', 'arrow', ''))}


def make(cfg, n):
    from gym_novel_gridworlds_amd import VecNovelGridworld, apply_novelty, make_spec
    env_id, S, nov = CFG[cfg]
    spec = make_spec(env_id, S)
    if nov:
        apply_novelty(spec, *nov)
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1, autoreset=True, horizon=100)
    v.reset()
    return v


def batched(args):
    import torch
    for cfg in CFG:
        v = make(cfg, args.n)
        os.environ['NGW_MASK_FUSED'] = '0'                  # (read at ngw_create: a second handle whose masks-on steps run the standalone kernel)
        v0 = make(cfg, args.n)
        os.environ.pop('NGW_MASK_FUSED')
        v0.set_action_masks(True)
        A = len(v.actions_id)
        acts = torch.randint(0, A, (64, args.n), dtype=torch.int32, device='cuda:0')
        torch.cuda.synchronize()
        res = {'off': [], 'fused': [], 'step_then_standalone': []}

        def run(form, k):
            e = v0 if form == 'step_then_standalone' else v
            if e is v:
                v.set_action_masks(form == 'fused')
            for t in range(k):
                e.step_device(acts[t % 64].data_ptr())
        for form in res:
            run(form, 30)
        v.sync(); v0.sync()
        for r in range(args.rounds):
            for form in res:
                e = v0 if form == 'step_then_standalone' else v
                e.sync()
                t0 = time.perf_counter()
                run(form, args.steps)
                e.sync()
                res[form].append((time.perf_counter() - t0) / args.steps * 1e6)
        out = {k: round(float(np.median(x)), 2) for k, x in res.items()}
        print(json.dumps({'figure': 'batched_step_us', 'cfg': cfg, 'n': args.n, 'steps': args.steps, 'rounds': args.rounds, **out,
                          'raw': {k: [round(y, 2) for y in x] for k, x in res.items()}}), flush=True)
        v.close(); v0.close()


def lean(args):
    """masks-off kernels the shared predicate touched: the step with the bit-row lidar at C2 / C3 and two EXT rollouts (before / after)"""
    import torch
    from gym_novel_gridworlds_amd import LidarInFront, VecNovelGridworld, apply_novelty, make_spec
    out = {'lib': os.environ.get('NGW_LIB', 'product')}
    for cfg in ('C2', 'C3'):
        v = make(cfg, args.n)
        w = LidarInFront(v, num_beams=8, dtype='packed')
        w.reset()
        acts = torch.randint(0, len(v.actions_id), (64, args.n), dtype=torch.int32, device='cuda:0')
        torch.cuda.synchronize()
        for t in range(30):
            v.step_device(acts[t % 64].data_ptr())
        v.sync()
        t0 = time.perf_counter()
        for t in range(args.steps):
            v.step_device(acts[t % 64].data_ptr())
        v.sync()
        out['lidar_step_us_' + cfg] = round((time.perf_counter() - t0) / args.steps * 1e6, 2)
        v.close()
    for name, env_id, S, nov in (('fire10h', 'NovelGridworld-Pogostick-v1', 10, ('firewall', 'hard', '', '')),
                                 ('fencer12h', 'NovelGridworld-Bow-v1', 12, ('fencerestriction', 'hard', 'jungle', ''))):
        spec = make_spec(env_id, S)
        apply_novelty(spec, *nov)
        v = VecNovelGridworld(spec=spec, num_envs=args.n, seed=1, autoreset=True, horizon=100)
        v.reset()
        v.rollout(50, action_seed=1)
        v.sync()
        t0 = time.perf_counter()
        v.rollout(500, action_seed=2)
        v.sync()
        out['rollout_G_env_steps_per_s_' + name] = round(args.n * 500 / (time.perf_counter() - t0) / 1e9, 2)
        v.close()
    print(json.dumps({'figure': 'touched_kernels', **out}), flush=True)


def host(args):
    v = make('C2', args.n)
    rs = np.random.RandomState(0)
    acts = rs.randint(0, len(v.actions_id), (64, args.n)).astype(np.int32)
    res = {'step': [], 'step_then_masks': []}
    for t in range(20):
        v.step(acts[t % 64])
    v.action_mask_words()
    for r in range(args.rounds):
        for form in res:
            t0 = time.perf_counter()
            for t in range(args.steps):
                v.step(acts[t % 64])
                if form == 'step_then_masks':
                    v.action_mask_words()
            res[form].append((time.perf_counter() - t0) / args.steps * 1e6)
    print(json.dumps({'figure': 'host_step_us', 'cfg': 'C2', 'n': args.n, **{k: round(float(np.median(x)), 2) for k, x in res.items()}}), flush=True)
    v.close()


def adapter(args):
    import gym_novel_gridworlds_amd as G
    res = {'step': [], 'masks_then_step': []}
    for r in range(args.rounds):
        for form in res:
            np.random.seed(0)
            env = G.make('NovelGridworld-Pogostick-v1')
            env.reset()
            for i in range(200):
                env.step(env.action_space.sample())
            t0 = time.perf_counter()
            for i in range(args.steps):
                if form == 'masks_then_step':
                    env.action_masks()
                env.step(env.action_space.sample())
                if (i + 1) % 1000 == 0:
                    env.reset()
            res[form].append(args.steps / (time.perf_counter() - t0))
            env.close()
    print(json.dumps({'figure': 'adapter_steps_per_s', **{k: round(float(np.median(x))) for k, x in res.items()}}), flush=True)


def c2(args):
    import torch
    v = make('C2', args.n)
    acts = torch.randint(0, 17, (64, args.n), dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    for t in range(50):
        v.step_device(acts[t % 64].data_ptr())
    v.sync()
    t0 = time.perf_counter()
    for t in range(args.steps):
        v.step_device(acts[t % 64].data_ptr())
    v.sync()
    print(json.dumps({'figure': 'c2_step_us', 'lib': os.environ.get('NGW_LIB', 'product'), 'n': args.n,
                      'us': round((time.perf_counter() - t0) / args.steps * 1e6, 2)}), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['batched', 'host', 'adapter', 'c2', 'lean'])
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    {'batched': batched, 'host': host, 'adapter': adapter, 'c2': c2, 'lean': lean}[a.what](a)
