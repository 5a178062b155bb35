"""tools/slot_observe_cost.py - what observing saved states by slot costs (include/ngw.h ngw_snapshot_lidar / ngw_snapshot_agent_view /
ngw_snapshot_action_mask), one JSON line per map size and count.

    python tools/slot_observe_cost.py [--counts 4096,65536] [--reps 20] [--rounds 5] [--cfgs C2,S32]

One child process per (configuration, count) (C2 Pogostick-v1 10 x 10, S32 Pogostick-v1 32 x 32), each under its own time limit; the first one
that fails ends the run.  `count` slots of one snapshot on a handle of `count` envs (the loop below cannot take more slots than envs), observed
through a random slot list with repeats - a device tensor -, into buffers allocated once.  After a warm-up, `rounds` rounds alternate the
variants; every figure is a HIP event pair on the env's stream around a window of `reps` repetitions (the average INCLUDING the gaps between
launches - what a caller's loop pays), reported as the median of the rounds with their minimum and maximum:
    slot_lidar / slot_view / slot_masks     the slot call: one launch, no env touched (lidar: int32 rows and packed rows)
    loop_lidar / loop_view / loop_masks     the loop it replaces: snapshot.restore(slots -> envs) + lidar_observation(device=True) / agent_view /
                                            action_mask_words + a copy of the rows + restoring the envs' own states from a second snapshot
The tool asserts that slot call and loop give the same rows, and reports us per call, bytes per row (read from the slot + written) and the
ratio loop / slot call.  No bar is set."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'C2': ('NovelGridworld-Pogostick-v1', 10), 'S32': ('NovelGridworld-Pogostick-v1', 32)}


def child(args):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld, _cabi, make_spec
    cfg, n = args.child, args.n
    env_id, S = CFG[cfg]
    spec = make_spec(env_id, S)
    A, V = len(spec.actions_id), 5
    W = 2 * V + 1
    dev = 'cuda:0'
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    warm = torch.randint(0, A, (20, n), dtype=torch.int32, device=dev, generator=g)
    slots = torch.randint(0, n, (n,), dtype=torch.int32, device=dev, generator=g)
    torch.cuda.synchronize()
    v = VecNovelGridworld(spec=spec, num_envs=n, seed=1)
    K = v.n_items
    v.reset()
    pool, own = v.snapshot(), v.snapshot()
    for t in range(warm.shape[0]):
        v.step_device(warm[t].data_ptr())
    pool.save()                                            # the nodes
    for t in range(5):
        v.step_device(warm[t].data_ptr())
    own.save()                                             # the envs' own states, which the loop has to put back
    v.sync()
    L = _cabi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    cur = lambda: torch.cuda.current_stream(0).cuda_stream   # noqa: E731
    pad = (n + 63) // 64 * 64
    view_s = torch.zeros((n * W * W + 3) // 4 * 4, dtype=torch.int8, device=dev)
    view_l = torch.zeros((n, W, W), dtype=torch.int8, device=dev)
    facing_s, inv_s = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, K), dtype=torch.int32, device=dev)
    masks_s, masks_l = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    rows = {}

    def loop(observe, dst):
        def run():
            pool.restore(slots=slots)
            dst.copy_(observe())                           # (the copy runs on torch's stream; the env's stream waits for it)
            v.stream_order(cur(), True)
            own.restore()
        return run

    def slot_view():
        _cabi.check(L.ngw_snapshot_agent_view(v._h, pool._s, ptr(slots), n, V, ptr(view_s), ptr(facing_s), ptr(inv_s)))

    def slot_masks():
        _cabi.check(L.ngw_snapshot_action_mask(v._h, pool._s, ptr(slots), n, ptr(masks_s)))
    variants = {'slot_view': slot_view, 'loop_view': loop(lambda: v.agent_view(V, device=True), view_l),
                'slot_masks': slot_masks, 'loop_masks': loop(lambda: v.action_mask_words(device=True), masks_l)}
    row_bytes = {'view': (S * S + 8 + 4 + 4 * K, W * W + 4 + 4 * K), 'masks': (14 + 8 + 4 + 1 + 4 * K, 8)}
    out = {'figure': 'slot_observe_cost', 'cfg': cfg, 'n': n, 'S': S, 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}

    def measure(variants):
        res = {k: [] for k in variants}
        for fn in variants.values():
            for _ in range(2):
                fn()
        v.sync()
        for r in range(args.rounds):
            for k, fn in variants.items():
                v.timing_begin()
                for _ in range(args.reps):
                    fn()
                res[k].append(v.timing_end() * 1e3 / args.reps)
        v.sync()
        torch.cuda.synchronize()
        for k, x in res.items():
            out[k] = {'us': round(float(np.median(x)), 1), 'min': round(float(min(x)), 1), 'max': round(float(max(x)), 1)}
    measure(variants)
    assert bool((view_s[:n * W * W].view(n, W, W) == view_l).all()), (cfg, 'view')
    assert bool((masks_s == masks_l).all()), (cfg, 'masks')
    for fmt, dtype in (('i32', np.int32), ('packed', 'packed')):
        v.lidar_configure(num_beams=8, dtype=dtype)
        rb = v.lidar_row_bytes
        rows_s = torch.zeros((pad, rb), dtype=torch.uint8, device=dev)
        rows_l = torch.zeros((n, rb), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def slot_lidar():
            _cabi.check(L.ngw_snapshot_lidar(v._h, pool._s, ptr(slots), n, ptr(rows_s)))

        def env_rows():
            o = v.lidar_observation(device=True)
            if isinstance(o, tuple):                       # packed: the two views of one buffer
                p = C.c_void_p()
                _cabi.check(L.ngw_lidar_device_ptr(v._h, C.byref(p)))
                from gym_novel_gridworlds_amd.vec_env import _DevArray
                return torch.as_tensor(_DevArray(p.value, (n, rb), '|u1'), device=dev)
            return o.view(torch.uint8).view(n, rb)
        measure({'slot_lidar_' + fmt: slot_lidar, 'loop_lidar_' + fmt: loop(env_rows, rows_l)})
        assert bool((rows_s[:n] == rows_l).all()), (cfg, 'lidar', fmt)
        row_bytes['lidar_' + fmt] = (S * S + 8 + 4 + 4 * K, rb)
    assert v.error_flags() == 0
    for k, (rd, wr) in row_bytes.items():
        out['slot_' + k]['B_per_row'] = rd + wr
        out['loop_over_slot_' + k] = round(out['loop_' + k]['us'] / out['slot_' + k]['us'], 2)
    print(json.dumps(out), flush=True)
    v.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', default='4096,65536')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cfgs', default='C2,S32')
    ap.add_argument('--limit', type=int, default=120, help='seconds per child')
    ap.add_argument('--child', default='')
    ap.add_argument('--n', type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    for cfg in a.cfgs.split(','):                         # (like `timeout ... && timeout ...`: nothing more starts after a failure)
        for n in a.counts.split(','):
            rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', cfg, '--n', n,
                                  '--reps', str(a.reps), '--rounds', str(a.rounds)])
            if rc:
                print(json.dumps({'figure': 'slot_observe_cost', 'cfg': cfg, 'n': int(n), 'failed': rc}), flush=True)
                sys.exit(rc)
