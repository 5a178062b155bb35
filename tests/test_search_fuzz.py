"""Randomised call sequences over the whole search surface of one handle, HIP path against the model of tests/search_fuzz.py: action masks,
snapshots (save, restore, copy, fork), expand, slot rollouts and playouts in every form, slot observers, lookahead, plan evaluation, state /
successor / path keys, the key table, weighted sampling, step_sampled, trajectories with lidar rows or AgentMap views (observe='agent_view', view
sizes 1 / 2 / 5 / 6, on rollout, playout and playouts) and a captured graph, interleaved with the steps, rollouts, resets and state injections of
tests/test_fuzz_parity.py - everything compared after every call, under drawn handle settings (prepared episodes and their depth, the small
page-locked block, env_index_base, fused lidar formats, masks in the step, terminal capture, batches that are no whole number of wavefronts).

Guided playouts (table=, table_weights=, outside=) run over the case's one key table as the other calls left it - keys inserted under other fields,
from other snapshots, possibly none - with limits, outside='stop', first_pair up to 2^40, from slots, from the envs and from another snapshot, with
children, every fields choice (KEY_INV alone among them: key 0), either observation, and a weight tensor whose rows outside the members' reported
buckets are NaN; actions, where, depth, reports, keys, rewards, masks, observations and the kept rows are the oracle's, and the table is as it was.
For the chunks in PROBED_CHUNKS the device's table must have placed a member outside its home bucket.

One case per configuration and chunk by default; NGW_FUZZ_SECONDS=<s> runs longer (a soak), NGW_FUZZ_SEED=<n> draws other sequences: a failure
message names the configuration, the case, the settings, the call's index and kind, and with the seed that reproduces it.  Six chunks: the model
side of one chunk, walked on the CPU against the stand-in (tests/test_search_fuzz_cpu.py; the stand-in computes everything a second time), was
measured at 3.7, 2.2, 2.5, 2.7, 2.8 and 2.4 s for the committed seed, with the per-call maxima as the issue set them (130 pairs, 8 steps, 3 plans);
on the MI355X a chunk takes 0.51 - 0.70 s (2.9 s for the first, which loads the library); before the guided kinds and the 'view' forms, measured in
the same session, 0.30 - 0.50 s (2.3 s for the first).

With the walk kinds, the frontier kinds and the padded device lists (IDX_NONE in a drawn subset of a call's index lists; search_fuzz.py's docstring),
cases of 8 - 15 calls and seed 7632, measured on one MI355X, seconds per chunk 0 .. 5:
    before (the parent's driver, seed 7100)   2.37  0.51  0.62  0.67  0.47  0.54
    after                                     3.39  0.76  0.74  0.77  0.96  0.70
and the CPU walk against the stand-in 4.0, 2.7, 3.2, 3.2, 3.3 and 2.4 s.  A soak of NGW_FUZZ_SECONDS=150 with NGW_FUZZ_SEED=9001
walked 2104 cases and passed.  Needs an MI355X."""
import os
import time

import numpy as np
import pytest

import search_fuzz as F

pytestmark = pytest.mark.gpu
CHUNKS = 6
BUDGET = float(os.environ.get('NGW_FUZZ_SECONDS', '0'))
SEED = int(os.environ.get('NGW_FUZZ_SEED', '7632'))        # (tests/test_fuzz_parity.py starts from 1000)
# the chunks of seed 7632 in which a guided call's table holds two members with one home bucket (tests/test_search_fuzz_cpu.py asserts the list from the
# model alone): there the device's table must report a member outside its home bucket - a probe chain the guided look-up has to walk
PROBED_CHUNKS = (0, 2, 3, 4, 5)


def make_env(**kw):
    import torch
    from gym_novel_gridworlds_amd import VecNovelGridworld
    v = VecNovelGridworld(**kw)

    def to_device(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        return t
    v.to_device, v.ptr_of = to_device, lambda t: t.data_ptr()
    return v


@pytest.mark.parametrize('chunk', range(CHUNKS))
def test_random_search_call_sequences_match_model(chunk):
    rs = np.random.RandomState(SEED + chunk)
    t_end = time.time() + (BUDGET / CHUNKS if BUDGET > 0 else 0)
    case = 0
    displaced = []

    def log(kind, status, form):
        if kind == '(guided)':
            displaced.append(dict(form)['displaced'])
    while True:
        for cfg in F.chunk_cfgs(chunk, CHUNKS):
            F.run_case(rs, cfg, case, make_env, log)
            case += 1
        if time.time() >= t_end:
            break
    if SEED == 7632 and chunk in PROBED_CHUNKS:
        assert sum(displaced) >= 1, "no guided call of this chunk met a member key outside its home bucket"
