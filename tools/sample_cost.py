"""tools/sample_cost.py - what the weighted choice among valid actions costs (include/ngw.h ngw_sample_actions) against the torch chain it
replaces, one JSON line per map size, env count and source.

    python tools/sample_cost.py [--envs 4096,65536] [--cfgs C2,S32] [--reps 3] [--rounds 5]

ONE process runs every shape, each shape after the other; the first one that fails ends the run.  `n` envs a few random steps after reset,
and a snapshot holding their states; float32 weights [A, n] on the device (a softmax of random logits).  After a warm-up, `rounds` rounds
alternate the variants; every figure is a HIP event pair on the env's stream around a window of `reps` repetitions (the average INCLUDING the
gaps between launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    sample        ngw_sample_actions: one launch (action, mass and mask word)
    chain         action_masks(device=True) (snap.action_masks(slots) from slots) -> the masked weights -> torch.multinomial -> a gather of the
                  chosen weight -> a sum for the mass
    step_sampled  env.step_sampled: the call + step_device, two launches, no host wait       (source = envs only)
    chain_step    the chain + step_device on its actions                                     (source = envs only)
The two draw from different generators, so they are not compared pair by pair; the tool asserts what must hold for both: every action is
valid for its state where any is, and the masses agree to float32 rounding.  No bar: the comparison is between the two on the same build."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}


def shape(args, cfg, n, source):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A = len(spec.actions_id)
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    weights = torch.softmax(torch.randn(A, n, device=dev, generator=g), 0).contiguous()
    slots = torch.randperm(n, device=dev, generator=g).to(torch.int32)
    act = torch.zeros(n, dtype=torch.int32, device=dev)
    mass = torch.zeros(n, dtype=torch.float32, device=dev)
    words = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    v.reset()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    pool = v.snapshot()
    pool.save()
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    from_slots = source == 'slots'
    out, tick = {}, [0]

    def sample():
        tick[0] += 1
        _cabi.check(L.ngw_sample_actions(v._h, pool._s if from_slots else None, ptr(slots) if from_slots else None, n, ptr(weights), n, 12345, 0,
                                         tick[0], ptr(act), ptr(mass), ptr(words)))

    def chain():
        ok = pool.action_masks(slots, device=True) if from_slots else v.action_masks(device=True)
        ok = torch.where(ok.any(1, keepdim=True), ok, torch.ones_like(ok))
        w = weights.t() * ok
        a = torch.multinomial(w, 1, generator=g)
        out['chain'] = (a.reshape(n).to(torch.int32), w.gather(1, a).reshape(n), w.sum(1), ok)

    def step_sampled():
        tick[0] += 1
        v.step_sampled(weights, 12345, t=tick[0])

    def chain_step():
        chain()
        v.stream_order(torch.cuda.current_stream(0).cuda_stream, True)        # the step reads what torch's stream is still writing
        v.step_device(out['chain'][0].data_ptr())

    variants = {'sample': sample, 'chain': chain}
    if not from_slots:
        variants.update(step_sampled=step_sampled, chain_step=chain_step)
    res = {k: [] for k in variants}
    for fn in (sample, chain):                          # the checks, on one state: before any variant steps the envs
        fn()
    v.sync()
    torch.cuda.synchronize()
    a_b, _, mass_b, ok = out['chain']
    assert bool(ok.gather(1, act.long()[:, None]).all()) and bool(ok.gather(1, a_b.long()[:, None]).all()), (cfg, n, source, 'an invalid action')
    assert bool(torch.allclose(mass, mass_b, rtol=1e-5, atol=0)), (cfg, n, source, 'masses')
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
            v.stream_order(torch.cuda.current_stream(0).cuda_stream, True)    # the window closes behind torch's share of the chain
            res[k].append(v.timing_end() * 1e3 / args.reps)
    v.sync()
    torch.cuda.synchronize()
    flags = v.error_flags()
    assert flags == 0, (cfg, n, source, 'error flags', flags)
    line = {'figure': 'sample_cost', 'cfg': cfg, 'S': S, 'envs': n, 'source': source, 'A': A, 'reps': args.reps, 'rounds': args.rounds,
            'device': torch.cuda.get_device_name(0)}
    for k, x in res.items():
        line[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    line['chain_over_sample'] = round(line['chain']['us'] / line['sample']['us'], 2)
    if not from_slots:
        line['chain_step_over_step_sampled'] = round(line['chain_step']['us'] / line['step_sampled']['us'], 2)
    print(json.dumps(line), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', default='4096,65536')
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--sources', default='envs,slots')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for cfg in a.cfgs.split(','):
        for n in a.envs.split(','):
            for source in a.sources.split(','):
                shape(a, cfg, int(n), source)
