"""tools/pairs_oracle_digest.py - one SHA-256 per (oracle function, case) of the six CPU reference models under tests/ that step saved rows:
oracle_slot_rollout, oracle_playout, oracle_weighted_playout, oracle_path, oracle_traj, oracle_guided.  No GPU.

    python tools/pairs_oracle_digest.py [--check]

Without --check the digests are written to tests/golden/pairs_oracle_digests.json; with it they are compared with that file (exit status 1 and
the labels that differ).  A digest covers every array a call returns - dtype, shape and bytes -, the `states` of every (step, pair) in sorted
order and the `events` counts, so a reference that moves by one bit anywhere shows.  tests/test_pairs_oracle_cpu.py recomputes them on every run.

The cases: the four configurations of guided_playout_oracle.CONFIGS, COUNT pairs drawn with repeats from twin(name)'s 20 rows, STEPS steps, under
the case seed SEEDS[name] (chosen so that the events tests/test_pairs_oracle_cpu.py asks for occur): limits that hold 0, STEPS and values in
between, plans that hold -1 and ids >= A, uniform and weighted playouts, guided playouts with `stop` on and off, with limits and with a lidar."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pairs_oracle_digests.json')
COUNT, STEPS = 24, 8
SEEDS = {'pogo10': 11, 'axe11': 12, 'fire12h': 13, 'pogo10lim': 14}
PLAY_SEED, FIRST_PAIR = 0x5EED0FCA5E5, 7


def feed(h, x):
    """Everything a result holds, in a fixed order."""
    if isinstance(x, dict):
        for k in sorted(x):
            h.update(repr(k).encode())
            feed(h, x[k])
    elif isinstance(x, (tuple, list)):
        h.update(b'(%d' % len(x))
        for v in x:
            feed(h, v)
    elif isinstance(x, np.ndarray):
        h.update(("%s%r" % (x.dtype.str, x.shape)).encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif x is None or isinstance(x, (bool, int, np.bool_, np.integer)):
        h.update(repr(None if x is None else int(x)).encode())
    else:
        raise TypeError("pairs_oracle_digest: %r in a result" % type(x))


def digest(result):
    h = hashlib.sha256()
    feed(h, result)
    return h.hexdigest()


def case_inputs(name):
    """-> dict: what every call of one configuration is given."""
    import guided_playout_oracle as GO
    spec, o, _, _, _ = GO.twin(name)
    _, _, auto, fields, _ = GO.CONFIGS[name]
    A = len(spec.actions_id)
    rs = np.random.RandomState(SEEDS[name])
    parents, default, members = GO.inputs(name, COUNT, STEPS)
    limits = rs.randint(0, STEPS + 1, COUNT)
    limits[:3] = (0, STEPS, STEPS // 2)
    plans = rs.randint(0, A, (STEPS, COUNT))                       # step-major
    odd = rs.rand(STEPS, COUNT)
    plans[odd < 0.08] = -1
    plans[odd > 0.92] = A + rs.randint(0, 3)
    plans[0, 3], plans[1, 4] = -1, A
    weights = (rs.randint(0, 5, A) * rs.randint(0, 2, A)).astype(np.float32)
    weights[rs.randint(A)] = 3.0
    return dict(spec=spec, rows=o.st, auto=auto, hz=GO.HORIZON if auto else 0, fields=fields, A=A, parents=parents, default=default, members=members,
                limits=limits, plans=plans, weights=weights, craft=GO.craft_ids(spec), lc=GO.lidar_cfg(name))


def results(names=None):
    """Yields (label, what the call returned) for every case."""
    import guided_playout_oracle as GO
    import path_key_oracle as KO
    import playout_oracle as PO
    import sample_oracle as SA
    import slot_rollout_oracle as RO
    import trajectory_oracle as TO
    for name in (GO.CONFIGS if names is None else names):
        c = case_inputs(name)
        spec, rows, p, auto, hz, f = c['spec'], c['rows'], c['parents'], c['auto'], c['hz'], c['fields']
        row_fn = lambda k, c=c: GO.row_of(k, c['A'], c['craft'])                                       # noqa: E731
        yield name + '/slot_rollout', RO.oracle_slot_rollout(spec, rows, p, c['plans'].T, auto, hz)
        play = PO.oracle_playout(spec, rows, p, STEPS, PLAY_SEED, FIRST_PAIR, auto, hz)
        yield name + '/playout', play
        wplay = SA.oracle_weighted_playout(spec, rows, p, STEPS, PLAY_SEED, c['weights'], FIRST_PAIR, auto, hz)
        yield name + '/weighted_playout', wplay
        yield name + '/path/plans+limits', KO.oracle_path(spec, rows, p, c['plans'], c['limits'], auto, hz, f)
        yield name + '/path/playout', KO.oracle_path(spec, rows, p, play[2], None, auto, hz, f)
        yield name + '/traj/plans+limits+lidar', TO.oracle_traj(spec, rows, p, c['plans'], c['limits'], auto, hz, f, c['lc'])
        yield name + '/traj/weighted_playout', TO.oracle_traj(spec, rows, p, wplay[2], None, auto, hz, f)
        yield name + '/guided', GO.oracle_guided(spec, rows, p, STEPS, PLAY_SEED, c['members'], row_fn, c['default'], FIRST_PAIR, auto, hz, f)
        yield name + '/guided/stop+limits', GO.oracle_guided(spec, rows, p, STEPS, PLAY_SEED, c['members'], row_fn, c['default'], FIRST_PAIR, auto, hz, f,
                                                              c['limits'], True)
        yield name + '/guided/lidar+no_default', GO.oracle_guided(spec, rows, p, STEPS, PLAY_SEED, c['members'], row_fn, None, 0, auto, hz, f, None, False,
                                                                  c['lc'])


def digests():
    return {label: digest(r) for label, r in results()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true')
    args = ap.parse_args()
    from oracle import ngw_oracle
    ngw_oracle.build()
    got = digests()
    text = json.dumps(got, indent=1, sort_keys=True) + '\n'
    if not args.check:
        with open(GOLDEN, 'w') as fh:
            fh.write(text)
        print("%d digests -> %s" % (len(got), os.path.relpath(GOLDEN, ROOT)))
        return 0
    with open(GOLDEN) as fh:
        want = json.load(fh)
    bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    print("%d digests, %d differ%s" % (len(got), len(bad), ''.join('\n  ' + k for k in bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
