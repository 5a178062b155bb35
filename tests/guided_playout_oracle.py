"""Expected guided playouts (playout(table=, table_weights=, outside=)) from the unmodified CPU oracle and the public numpy contracts: a forward
simulation.  Per step of the pairs still alive: the key of the row each pair is in (state_keys.keys_of_rows on the oracle's rows), membership of that
key in the table - modelled as a SET of keys -, the weights (a function f(key) of the key where it is a member, the default vector or zeros where
not), the mask word (trajectory_oracle.mask_words: the mask oracle with the all-actions replacement), the playout's Philox word
(playout.playout_words), the weighted choice (sample.choose_weighted) - a chooser - and one step of pairs_oracle.step_pairs, whose record holds
everything else a result does - reports, keys, rewards, end rows, the rows visited -; the observations are trajectory_oracle.observed's on those rows.
The oracle needs no bucket numbers: the tests write f(key) into row where_of(key) after the insert, and compare the `where`
output with what insert / lookup returned.  Nothing here uses the device's own step, mask, key, probe or choice."""
import functools

import numpy as np

import expand_oracle as XO
import ngw_testlib as T
import pairs_oracle as PA
import path_key_oracle as KO
import playout_oracle as PO
import trajectory_oracle as TO
from gym_novel_gridworlds_amd.playout import playout_words
from gym_novel_gridworlds_amd.sample import bad_weights, choose_weighted
from gym_novel_gridworlds_amd.state_keys import KEY_STATE, KEY_STEP_COUNT, keys_of_rows, mix64
from oracle.ngw_oracle import Oracle

STATE_KEYS = PA.STATE_KEYS
COUNT, STEPS, N, HORIZON = 130, 12, 20, 9           # two full waves and two lanes, repeated parents
SEED, FILL_SEED = 0x6D1DED0123456789, 0x7AB1E5EED0000001
LIMITED = ('Break', 'Forward', 'Left', 'Right', 'Craft_plank', 'Craft_stick')
# name -> (ngw_testlib configuration, map size, autoreset with HORIZON, key fields, the limited action list or None)
CONFIGS = {'pogo10': ('pogo10', 10, False, KEY_STATE, None),
           'axe11': ('axe10', 11, False, KEY_STATE, None),                                  # S * S = 121: no multiple of 4; pick-ups rebuild the map part
           'fire12h': ('fire10h', 12, True, KEY_STATE | KEY_STEP_COUNT, None),              # deaths, horizon cuts, the step count in the key
           'pogo10lim': ('pogo10', 10, False, KEY_STATE, LIMITED)}                          # the action table LimitActions' playouts run on


def row_of(key, n_actions, craft):
    """f(key): the weight row of a member key - a function of the key alone.  Peaked on one action, all zero, weight on crafting actions only
    (invalid without the ingredients), or a spread of small integers."""
    k, x = int(key), np.zeros(n_actions, np.float32)
    kind = (k >> 3) % 5
    if kind in (0, 4):
        x[(k >> 11) % n_actions] = 1 + (k >> 20) % 7
    elif kind == 2:
        x[craft if len(craft) else [n_actions - 1]] = 2.0
    elif kind == 3:
        x[:] = [(k >> (5 + 3 * (a % 19))) & 7 for a in range(n_actions)]
    return x                                            # (kind 1: all zero)


def build_spec(name):
    cfg, size, _, _, limited = CONFIGS[name]
    spec = T.build_spec(cfg, map_size=size)
    if limited is not None:
        from gym_novel_gridworlds_amd.wrappers import limited_spec
        spec = limited_spec(spec, limited)
    return spec


@functools.lru_cache(maxsize=None)
def twin(name, n=N, warm=10):
    """The oracle after `warm` random steps (step counters spread over the horizon under autoreset), and what a device env needs to be its twin."""
    _, _, auto, _, _ = CONFIGS[name]
    spec = build_spec(name)
    seed = XO.good_seed(spec, n)
    kw = dict(autoreset=True, horizon=HORIZON) if auto else {}
    o = Oracle(spec.compile(), n, seed=seed, **kw)
    o.reset()
    rs = np.random.RandomState(n + warm)
    warmup = [rs.randint(0, len(spec.actions_id), n).astype(np.int32) for _ in range(warm)]
    for a in warmup:
        o.step(a)
    if auto:
        o.st.step_count[...] = np.arange(n) % HORIZON
    return spec, o, seed, kw, warmup


def lidar_cfg(name, beams=8):
    """The LidarConfig of a configuration in the reference's order: the item set is fixed on the plain env of that size."""
    from gym_novel_gridworlds_amd.lidar import LidarConfig
    from gym_novel_gridworlds_amd.spec import make_spec
    cfg, size, _, _, _ = CONFIGS[name]
    return LidarConfig(make_spec(T.CFGS[cfg][0], size), beams)


def craft_ids(spec):
    return sorted(i for a, i in spec.actions_id.items() if a.startswith('Craft_'))


@functools.lru_cache(maxsize=None)
def inputs(name, count=COUNT, steps=STEPS):
    """-> (parents [count] with repeats, default weights [A], the member keys: uint64, distinct, in first-seen order).  The members are the keys
    of the parents and of the even steps of a PLAIN playout from the same parents under FILL_SEED."""
    spec, o, _, _, _ = twin(name)
    _, _, auto, fields, _ = CONFIGS[name]
    rs = np.random.RandomState(len(name) * 1000 + count)
    parents = rs.randint(0, N, count)
    A = len(spec.actions_id)
    default = (rs.randint(0, 4, A) * rs.randint(0, 2, A)).astype(np.float32)
    default[rs.randint(A)] = 1.0
    hz = HORIZON if auto else 0
    _, _, acts, _ = PO.oracle_playout(spec, o.st, parents, steps, FILL_SEED, 0, auto, hz)
    keys, _, _, _, _ = KO.oracle_path(spec, o.st, parents, acts, None, auto, hz, fields)
    own = keys_of_rows(PA.rows_of(XO.rows_state(spec, o.st, parents)), fields)
    offered = np.concatenate([own, keys[0::2].reshape(-1)])              # (the even steps' path keys: the states steps 0, 2, .. leave)
    members = []
    seen = set()
    for k in offered.tolist():
        if k and k not in seen:
            seen.add(k)
            members.append(k)
    return parents, default, np.array(members, np.uint64)


def oracle_guided(spec, rows, parents, steps, seed, members, row_fn, default=None, first_pair=0, autoreset=False, horizon=0, fields=KEY_STATE, limits=None,
                  stop=False, lc=None):
    """-> oracle_traj's dict for the actions the rule chooses, with 'actions' int32 [T, count] (-1: not executed), 'before' uint64 [T, count] (the key
    looked up at every executed step, 0 elsewhere), 'hit' bool [T, count], 'depth' int32 [count], 'bad' (a row that was read holds a bad weight) and
    'events' extended by the coverage counts: hits, misses, executed, reentries (pairs), zero_mass (in-table steps whose row had mass 0), differs
    (in-table steps whose action is not what the default weights give on the same word)."""
    A = spec.compile().n_actions
    member = set(int(k) for k in np.asarray(members, np.uint64).tolist())
    dflt = np.zeros(A, np.float32) if default is None else np.asarray(default, np.float32)
    ev = dict(zero_mass=0, differs=0, bad=False)

    def choose(t, idx, now):
        """The guided rule on the rows the pairs are in: the table look-up, `stop`, the weighted choice on the playout's own Philox word."""
        keys = keys_of_rows(now, fields)
        inside = np.array([int(k) in member for k in keys.tolist()], bool)
        on = inside if stop else np.ones(len(idx), bool)
        a, m = np.full(len(idx), -1, np.int32), np.zeros(len(idx), np.uint64)
        if on.any():
            m[on] = TO.mask_words(spec, {k: now[k][on] for k in STATE_KEYS})
            W = np.stack([row_fn(k) if h else dflt for k, h in zip(keys[on].tolist(), inside[on])]).astype(np.float32)
            ev['bad'] = ev['bad'] or bad_weights(W)
            pairs = (first_pair + idx[on]).astype(np.uint64)
            words = playout_words(seed, pairs, t)
            a[on], mass, _ = choose_weighted(m[on], W, seed, pairs, t, A, words=words)
            a_default, _, _ = choose_weighted(m[on], np.broadcast_to(dflt, W.shape), seed, pairs, t, A, words=words)
            ev['zero_mass'] += int((inside[on] & (mass == 0)).sum())
            ev['differs'] += int((inside[on] & (a[on] != a_default)).sum())
        return a, dict(stop=~on, masks=m, before=keys, hit=inside)

    e = TO.observed(spec, PA.step_pairs(spec, rows, parents, steps, choose, limits, autoreset, horizon, fields, record=True), lc, masks=False)
    ran, length = e.pop('ran'), e['reports']['length']
    hit = PA.kept(e, 'hit', bool)
    reentries = 0
    for j in range(len(length)):
        h = hit[:length[j], j]
        miss = np.nonzero(~h)[0]
        reentries += int(miss.size > 0 and h[miss[0]:].any())
    e['events'].update(zero_mass=ev['zero_mass'], differs=ev['differs'], hits=int(hit.sum()), misses=int((~hit & ran).sum()), executed=int(ran.sum()),
                       reentries=reentries)
    e.update(masks=PA.kept(e, 'masks', np.uint64), before=PA.kept(e, 'before', np.uint64), hit=hit, depth=np.cumprod(hit, 0).sum(0).astype(np.int32),
             bad=bool(ev['bad']))
    del e['parent_rows']
    return e


@functools.lru_cache(maxsize=None)
def expected(name, stop=False, weighted=True, lidar=False, count=COUNT, steps=STEPS):
    """The oracle's side of one configuration's parity case, computed once and shared (nobody writes to it)."""
    spec, o, _, _, _ = twin(name)
    _, _, auto, fields, _ = CONFIGS[name]
    parents, default, members = inputs(name, count, steps)
    A, craft = len(spec.actions_id), craft_ids(spec)
    lc = lidar_cfg(name) if lidar else None
    return oracle_guided(spec, o.st, parents, steps, SEED, members, lambda k: row_of(k, A, craft), default if weighted else None, 0, auto,
                         HORIZON if auto else 0, fields, None, stop, lc)


def coverage(e):
    """The coverage conditions of a parity case under the oracle alone; -> the event counts."""
    ev = e['events']
    assert ev['hits'] >= 0.2 * ev['executed'], ev
    assert ev['misses'] >= 0.2 * ev['executed'], ev
    assert ev['reentries'] >= 1 and ev['zero_mass'] >= 1 and ev['differs'] >= 1, ev
    return ev


def home_buckets(keys, buckets):
    """mix64(key) & mask on the host: where a key's probe starts."""
    return (mix64(np.asarray(keys, np.uint64)) & np.uint64(buckets - 1)).astype(np.int64)


def rows_for(keys, where, buckets, n_actions, craft, fill=0.0):
    """The [buckets, A] weight tensor of the tests: row where[i] = f(keys[i]), every other row `fill`."""
    tw = np.full((buckets, n_actions), fill, np.float32)
    for k, b in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(where).tolist()):
        assert 0 <= b < buckets
        tw[b] = row_of(k, n_actions, craft)
    return tw
