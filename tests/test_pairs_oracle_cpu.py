"""The CPU reference models that step saved rows did not move: every result of the six public oracle functions over pairs_oracle.step_pairs, on the
cases of tools/pairs_oracle_digest.py, hashes to what tests/golden/pairs_oracle_digests.json recorded before the six loops became one - and those
cases meet what the loops differ on: deaths, horizon cuts, limits, no-op ids, pick-ups, guided steps inside and outside the table.  No GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'pairs_oracle_digest.py')


@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('pairs_oracle_digest', TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def results(tool):
    return dict(tool.results())


def events_of(result):
    if isinstance(result, dict):
        return result['events']
    return result[4] if len(result) == 5 else {}                  # (oracle_path's tuple; the plain oracles return no counts)


def test_the_digests_are_the_recorded_ones(tool, results):
    with open(tool.GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(results) == sorted(want)
    moved = sorted(label for label, r in results.items() if tool.digest(r) != want[label])
    assert not moved, "the reference moved in %d of %d cases: %s" % (len(moved), len(want), moved)


def test_a_digest_sees_one_bit(tool, results):
    ends, rep, alive = results['pogo10/slot_rollout']
    flipped = dict(rep, info=rep['info'] ^ np.uint32(1 << 31) * (np.arange(len(rep['info'])) == 5).astype(np.uint32))
    assert tool.digest((ends, flipped, alive)) != tool.digest((ends, rep, alive))


def test_the_cases_meet_what_the_loops_differ_on(tool, results):
    total = {}
    for label, r in results.items():
        for k, v in events_of(r).items():
            total[k] = total.get(k, 0) + v
    assert total['deaths'] >= 1 and total['cuts'] >= 1 and total['limited'] >= 1 and total['pickups'] >= 1, total
    assert total['hits'] >= 1 and total['misses'] >= 1, total
    fire = events_of(results['fire12h/path/playout'])
    assert fire['deaths'] >= 1 and fire['cuts'] >= 1, fire            # a FireWall death and a horizon cut, under autoreset with the horizon
    noops = 0
    for name in tool.SEEDS:
        c = tool.case_inputs(name)
        plans, limits = c['plans'], c['limits']
        assert (plans == -1).any() and (plans >= c['A']).any()
        assert (limits == 0).any() and (limits == tool.STEPS).any() and ((limits > 0) & (limits < tool.STEPS)).any()
        assert len(set(c['parents'].tolist())) < len(c['parents']) == tool.COUNT
        _, rep, _, _, ev = results[name + '/path/plans+limits']
        executed = np.arange(tool.STEPS)[:, None] < rep['length'][None, :]
        noops += int((executed & ((plans < 0) | (plans >= c['A']))).sum())
        assert ev['limited'] >= 1, (name, ev)
        stopped, free = events_of(results[name + '/guided/stop+limits']), events_of(results[name + '/guided'])
        assert stopped['misses'] == 0 and stopped['hits'] >= 1 and free['hits'] >= 1 and free['misses'] >= 1, (name, stopped, free)
    assert noops >= 1
