"""Shared helpers for the parity tests: fixture loading, configuration table, and replay drivers that run the
SAME checks against any backend exposing `load / step / state` (the CPU oracle here, the HIP path in -m gpu)."""
import json
import os

import numpy as np

from gym_novel_gridworlds_amd.novelty import apply_novelty
from gym_novel_gridworlds_amd.spec import STEP_COSTS, make_spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
POGO, BOW = 'NovelGridworld-Pogostick-v1', 'NovelGridworld-Bow-v1'

# must match tests/golden/gen_golden.py CFGS
CFGS = {
    'pogo10': (POGO, 10, None), 'bow20': (BOW, 20, None),
    'axe10': (POGO, 10, ('axe', 'medium', 'wooden', '')), 'add32': (POGO, 32, ('additem', 'hard', 'arrow', '')),
    'pogo13': (POGO, 13, None), 'bow10': (BOW, 10, None), 'axe12bi': (POGO, 12, ('axe', 'medium', 'iron', 'true')),
    'add12m': (POGO, 12, ('additem', 'medium', 'spring', '')), 'add11e': (POGO, 11, ('additem', 'easy', 'arrow', '')),
    'bowaxe16': (BOW, 16, ('axe', 'medium', 'wooden', 'false')),
    'axeeasy10': (POGO, 10, ('axe', 'easy', 'wooden', '')),
    'brkinc10': (POGO, 10, ('breakincrease', 'hard', '', '')), 'brkinclog12': (POGO, 12, ('breakincrease', 'hard', 'tree_log', '')),
    'extdec10': (BOW, 10, ('extractincdec', 'hard', 'decrease', '')), 'axetbe10': (POGO, 10, ('axetobreak', 'easy', 'wooden', '')),
    'axetbm12': (BOW, 12, ('axetobreak', 'medium', 'iron', '')), 'remape10': (POGO, 10, ('remapaction', 'easy', '', '')),
    'remapm10': (BOW, 10, ('remapaction', 'medium', '', '')), 'remaph10': (POGO, 10, ('remapaction', 'hard', '', '')),
    'chop10': (POGO, 10, ('addchop', 'hard', '', '')), 'jump12': (BOW, 12, ('addjump', 'hard', '', '')),
    'pogov0_10': ('NovelGridworld-Pogostick-v0', 10, None),
    'pogov0_14': ('NovelGridworld-Pogostick-v0', 14, ('axe', 'medium', 'wooden', '')),
    'bowv0_12': ('NovelGridworld-Bow-v0', 12, None),
    'axehard10': (POGO, 10, ('axe', 'hard', 'wooden', '')), 'axehardi12': (BOW, 12, ('axe', 'hard', 'iron', 'true')),
    'atbhard10': (POGO, 10, ('axetobreak', 'hard', 'wooden', '')), 'atbhardi11': (BOW, 11, ('axetobreak', 'hard', 'iron', '')),
    'fence10e': (POGO, 10, ('fence', 'easy', 'oak', '')), 'fence12h': (BOW, 12, ('fence', 'hard', 'jungle', '')),
    'fencer10e': (POGO, 10, ('fencerestriction', 'easy', 'oak', '')), 'fencer10m': (POGO, 10, ('fencerestriction', 'medium', 'oak', '')),
    'fencer12h': (BOW, 12, ('fencerestriction', 'hard', 'jungle', '')), 'repl10m': (POGO, 10, ('replaceitem', 'medium', 'tree_log', 'brick')),
    'replwall12e': (BOW, 12, ('replaceitem', 'easy', 'wall', 'brick')), 'fire10h': (POGO, 10, ('firewall', 'hard', '', '')),
    'fire14m': (BOW, 14, ('firewall', 'medium', '', '')), 'crate10m': (POGO, 10, ('crate', 'medium', '', '')),
    'crate12h': (BOW, 12, ('crate', 'hard', '', '')), 'crate11e': (POGO, 11, ('crate', 'easy', '', '')),
}
CFGS.update({
    'stk_axe_bi10': (POGO, 10, [('axe', 'medium', 'wooden', ''), ('breakincrease', 'hard', '', '')]),
    'stk_bi_axe10': (POGO, 10, [('breakincrease', 'hard', 'tree_log', ''), ('axe', 'medium', 'iron', 'true')]),
    'stk_add_axe12': (POGO, 12, [('additem', 'easy', 'arrow', ''), ('axe', 'easy', 'wooden', '')]),
    'stk_atb_bi11': (BOW, 11, [('axetobreak', 'easy', 'iron', ''), ('breakincrease', 'hard', '', '')]),
    'stk_fen_fire12': (POGO, 12, [('fence', 'easy', 'oak', ''), ('firewall', 'medium', '', '')]),
    'stk_add_repl12': (BOW, 12, [('additem', 'medium', 'arrow', ''), ('replaceitem', 'medium', 'arrow', 'dart')]),
    'stk_fire_axe10': (POGO, 10, [('firewall', 'medium', '', ''), ('axe', 'medium', 'wooden', '')]),
    'stk_fire_axeh10': (POGO, 10, [('firewall', 'medium', '', ''), ('axe', 'hard', 'wooden', '')]),
    'stk_fr_axe10': (POGO, 10, [('fencerestriction', 'hard', 'oak', ''), ('axe', 'easy', 'wooden', '')]),
    'stk_axe_fr10': (POGO, 10, [('axe', 'easy', 'wooden', ''), ('fencerestriction', 'medium', 'oak', '')]),
    'stk_crate_fr12': (BOW, 12, [('crate', 'medium', '', ''), ('fencerestriction', 'hard', 'oak', '')]),
    'stk_fr_crate12': (BOW, 12, [('fencerestriction', 'hard', 'oak', ''), ('crate', 'medium', '', '')]),
    'stk_crate_bi10': (POGO, 10, [('crate', 'hard', '', ''), ('breakincrease', 'hard', '', '')]),
    'stk_add_crate12': (POGO, 12, [('additem', 'medium', 'arrow', ''), ('crate', 'medium', '', '')]),
    'stk_crate_add12': (BOW, 12, [('crate', 'hard', '', ''), ('additem', 'easy', 'arrow', '')]),
    'stk_fen_fr12': (POGO, 12, [('fence', 'easy', 'oak', ''), ('fencerestriction', 'hard', 'jungle', '')]),
    'stk_fr_fen12': (BOW, 12, [('fencerestriction', 'medium', 'oak', ''), ('fence', 'medium', 'jungle', '')]),
    'stk_repl_fire12': (POGO, 12, [('replaceitem', 'medium', 'crafting_table', 'anvil'), ('firewall', 'hard', '', '')]),
    'stk_fire_repl12': (BOW, 12, [('firewall', 'medium', '', ''), ('replaceitem', 'hard', 'wool', 'silk')]),
})
# configurations WITHOUT reference fixtures (larger maps of pinned components: the oracle is the checker there)
CFGS.update({'fire32m': (POGO, 32, ('firewall', 'medium', '', '')), 'fencer24h': (BOW, 24, ('fencerestriction', 'hard', 'oak', '')),
             'repl40e': (POGO, 40, ('replaceitem', 'easy', 'wall', 'brick'))})
# AddItem at every mask width of the new-episode kernel (register masks of 2 / 8 words, LDS masks) and beyond the packed array
CFGS.update({'add18h': (BOW, 18, ('additem', 'hard', 'arrow', '')), 'add24m': (POGO, 24, ('additem', 'medium', 'arrow', '')),
             'add29h': (BOW, 29, ('additem', 'hard', 'spring', '')), 'add36e': (POGO, 36, ('additem', 'easy', 'arrow', '')),
             'crate20h': (POGO, 20, ('crate', 'hard', '', ''))})
NO_FIXTURES = ('fire32m', 'fencer24h', 'repl40e', 'add18h', 'add24m', 'add29h', 'add36e', 'crate20h')
REMAP_SEED = {'remape10': 11, 'remapm10': 12, 'remaph10': 13, 'crate10m': 31, 'crate12h': 32, 'crate11e': 33,
              'stk_crate_fr12': 34, 'stk_fr_crate12': 35, 'stk_crate_bi10': 36, 'stk_add_crate12': 37, 'stk_crate_add12': 38, 'crate20h': 39}
HEADLINE = ['pogo10', 'bow20', 'axe10', 'add32']       # BASELINE.json configs 2-5

_spec_json = None
_npz = {}


def spec_json():
    global _spec_json
    if _spec_json is None:
        _spec_json = json.load(open(os.path.join(GOLDEN, 'spec.json')))
    return _spec_json


def golden(cfg):
    if cfg not in _npz:
        _npz[cfg] = dict(np.load(os.path.join(GOLDEN, cfg + '.npz')))
    return _npz[cfg]


def build_spec(cfg, map_size=None):
    env_id, S, nov = CFGS[cfg]
    spec = make_spec(env_id, S if map_size is None else map_size)
    if nov is not None:
        if cfg in REMAP_SEED:
            state = np.random.get_state()
            np.random.seed(REMAP_SEED[cfg])       # same global-stream position as the reference had at injection
        for one in novelty_list(nov):                # a stack: injected in order, the last one is the outermost wrapper
            apply_novelty(spec, *one)
        if cfg in REMAP_SEED:
            np.random.set_state(state)
    return spec


def novelty_list(nov):
    return [] if nov is None else ([nov] if isinstance(nov[0], str) else [tuple(x) for x in nov])


def messages():
    return spec_json()['messages']


class OracleBackend:
    """n envs on the CPU oracle."""

    def __init__(self, spec, n, **kw):
        from oracle.ngw_oracle import Oracle
        self.spec = spec
        self.o = Oracle(spec.compile(), n, **kw)
        self.n = n

    def load(self, i, map_, loc, facing, inv=None, sel=0, step_count=0):
        st = self.o.st
        st.map[i] = map_
        st.loc[i] = loc
        st.facing[i] = facing
        st.inv[i] = 0 if inv is None else inv
        st.selected[i] = sel
        st.step_count[i] = step_count

    def load_all(self, map_, loc, facing, inv, sel):
        st = self.o.st
        st.map[...], st.loc[...], st.facing[...], st.inv[...], st.selected[...] = map_, loc, facing, inv, sel
        st.step_count[...] = 0

    def add_inventory(self, i, item, q):
        self.o.st.inv[i, item] += q

    def step(self, actions):
        flags = self.o.step(actions)
        o = self.o
        return dict(flags=flags, reward=o.reward.copy(), done=o.done.copy(), result=o.result, cost_code=o.cost_code,
                    msg_code=o.msg_code, msg_arg=o.msg_arg)

    def state(self):
        st = self.o.st
        return dict(map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, sel=st.selected, step_count=st.step_count)


def check_outs(spec, out, idx, action, g_reward, g_done, g_result, g_cost, g_cost_is_int, g_msg, where):
    """Compare decoded step outputs of env idx with the golden scalars."""
    cost = STEP_COSTS[int(out['cost_code'][idx])]
    msg = spec.format_message(int(action), int(out['msg_code'][idx]), int(out['msg_arg'][idx]))
    got = (int(out['reward'][idx]), int(out['done'][idx]), int(out['result'][idx]), float(cost), int(type(cost) is int), msg)
    exp = (int(g_reward), int(g_done), int(g_result), float(g_cost), int(g_cost_is_int), messages()[int(g_msg)])
    assert got == exp, "%s: action %d -> got %r expected %r" % (where, action, got, exp)


class RefStackedStepCount:
    """What the REFERENCE's `env.step_count` does under two stacked novelty wrappers - the one documented deviation of this build
    (DESIGN.md "Not reproduced, on purpose"), as an explicit model the golden replay holds the recorded reference values to.
    gym.Wrapper forwards attribute READS to the env it wraps, not writes: a wrapper whose own step() epilogue runs
    `self.env.step_count += 1` (novelty_wrappers.py:199 AxeMedium, :966 FenceRestriction, ...; the axe / axetobreak / breakincrease
    wrappers handle Break - and the craftable axe's Craft action - without calling the env they wrap, FenceRestriction medium / hard
    calls it first when the Break is allowed) READS the counter through the wrapper below it and WRITES the result onto that wrapper
    object, where it shadows the env's counter from then on; `set_lasts` then copies that stale shadow + 1 over the env's counter.
    This build's counter is the un-shadowed one: +1 per step, +2 for a FenceRestriction Break that went through (:966)."""

    def __init__(self, novs, spec):
        self.W = []
        brk = spec.actions_id.get('Break')
        for name, diff, _a1, _a2 in novs:                                # bottom-up: injection order
            if name in ('axe', 'axetobreak', 'breakincrease'):
                ids = {brk}
                if name != 'breakincrease' and diff == 'hard':
                    ids |= {i for n, i in spec.actions_id.items() if n.startswith('Craft_') and n.endswith('_axe')}
                self.W.append(('handler', ids))
            elif name == 'fencerestriction' and diff != 'easy':
                self.W.append(('fr', {brk}))
            else:
                self.W.append(('pass', set()))
        self.E, self.shadow = 0, [None] * len(self.W)

    def _read(self, i):                                                  # `wrapper_i.step_count`: its own shadow, else the next object down
        while i >= 0:
            if self.shadow[i] is not None:
                return self.shadow[i]
            i -= 1
        return self.E

    def _epilogue(self, i):                                              # wrapper i: `self.env.step_count += 1`, then set_lasts
        if i == 0:
            self.E += 1                                                  # (self.env IS the base env: a real increment)
        else:
            self.shadow[i - 1] = self._read(i - 1) + 1
            self.E = self.shadow[i - 1]

    def _step(self, i, a, went_through):
        if i < 0:
            self.E += 1                                                  # pogostick_v1_env.py:362
            return
        kind, ids = self.W[i]
        if kind == 'handler' and a in ids:
            self._epilogue(i)
        elif kind == 'fr' and a in ids:
            if went_through:
                self._step(i - 1, a, went_through)
            self._epilogue(i)
        else:
            self._step(i - 1, a, went_through)

    def reset(self):
        self.E = 0                                                       # (the shadows stay: nothing ever deletes them)

    def step(self, action, went_through):
        self._step(len(self.W) - 1, int(action), went_through)
        return self.E


def replay_traces(cfg, backend_cls, **kw):
    """G3: all traces of a configuration in lock-step, one env per trace."""
    g = golden(cfg)
    spec = build_spec(cfg)
    stacked = [RefStackedStepCount(CFGS[cfg][2], spec) for _ in range(spec_json()['cfgs'][cfg]['n_traces'])] if cfg.startswith('stk_') else None
    ntr = spec_json()['cfgs'][cfg]['n_traces']
    T = spec_json()['cfgs'][cfg]['trace_len']
    S2 = spec.map_size ** 2
    be = backend_cls(spec, ntr, **kw)
    exp_map = np.zeros((ntr, S2), np.int8)
    ev = []
    for k in range(ntr):
        p = 'tr%d_' % k
        ev.append(dict(rl={int(t): j for j, t in enumerate(g[p + 'rl_t'])},
                       inj={}, md={}))
        for t, it, q in zip(g[p + 'inj_t'], g[p + 'inj_item'], g[p + 'inj_q']):
            ev[k]['inj'].setdefault(int(t), []).append((int(it), int(q)))
        for t, i, v in zip(g[p + 'md_t'], g[p + 'md_i'], g[p + 'md_v']):
            ev[k]['md'].setdefault(int(t), []).append((int(i), int(v)))
    acts = np.stack([g['tr%d_action' % k] for k in range(ntr)], 1)      # [T, ntr]
    prev_sc = np.zeros(ntr, np.int64)
    for t in range(T):
        for k in range(ntr):
            p = 'tr%d_' % k
            if t in ev[k]['rl']:
                j = ev[k]['rl'][t]
                be.load(k, g[p + 'rl_map'][j], g[p + 'rl_loc'][j], g[p + 'rl_facing'][j],
                        inv=g[p + 'rl_inv'][j] if p + 'rl_inv' in g else None)
                exp_map[k] = g[p + 'rl_map'][j]
                if stacked:
                    stacked[k].reset()
                    prev_sc[k] = 0
            for it, q in ev[k]['inj'].get(t, ()):
                be.add_inventory(k, it, q)
        out = be.step(acts[t])
        assert out['flags'] == 0
        st = be.state()
        for k in range(ntr):
            p = 'tr%d_' % k
            where = '%s trace %d step %d' % (cfg, k, t)
            check_outs(spec, out, k, acts[t, k], g[p + 'reward'][t], g[p + 'done'][t], g[p + 'result'][t],
                       g[p + 'cost'][t], g[p + 'cost_is_int'][t], g[p + 'msg'][t], where)
            for i, v in ev[k]['md'].get(t, ()):
                exp_map[k, i] = v
            assert (st['loc'][k] == g[p + 'loc'][t]).all() and st['facing'][k] == g[p + 'facing'][t], where
            assert st['sel'][k] == g[p + 'sel'][t] and (st['inv'][k] == g[p + 'inv'][t]).all(), where
            if stacked is None:
                assert st['step_count'][k] == g[p + 'step_count'][t], where
            else:
                # Stacked wrappers, the documented deviation held explicitly: this build's counter advances by 1 (2 for a
                # FenceRestriction Break that went through), and the value the REFERENCE recorded is what the write-shadowing model
                # above makes of the same steps - so the two differ exactly where, and by how much, DESIGN.md says they do.
                inc = int(st['step_count'][k]) - int(prev_sc[k])
                assert inc in (1, 2), where
                assert stacked[k].step(acts[t, k], inc == 2) == g[p + 'step_count'][t], where + ' (reference step_count model)'
                prev_sc[k] = st['step_count'][k]
        assert (st['map'] == exp_map).all(), '%s step %d map mismatch' % (cfg, t)
    return ntr * T


def replay_single_steps(cfg, backend_cls, **kw):
    """G4: every injected-state case as its own env, one batched step."""
    g = golden(cfg)
    spec = build_spec(cfg)
    n = len(g['ss_action'])
    be = backend_cls(spec, n, **kw)
    be.load_all(g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    out = be.step(g['ss_action'])
    assert out['flags'] == 0
    st = be.state()
    exp_map = g['ss_pre_map'].copy()
    exp_map[g['ss_md_c'], g['ss_md_i']] = g['ss_md_v']
    for c in range(n):
        check_outs(spec, out, c, g['ss_action'][c], g['ss_reward'][c], g['ss_done'][c], g['ss_result'][c],
                   g['ss_cost'][c], g['ss_cost_is_int'][c], g['ss_msg'][c], '%s single-step case %d' % (cfg, c))
    assert (st['loc'] == g['ss_post_loc']).all() and (st['facing'] == g['ss_post_facing']).all()
    assert (st['sel'] == g['ss_post_sel']).all() and (st['inv'] == g['ss_post_inv']).all()
    assert (st['map'] == exp_map).all()
    return n


def replay_solved(cfg, backend_cls, **kw):
    """G5: scripted-solver episodes, one env per episode (ragged lengths: shorter ones idle on Left)."""
    g = golden(cfg)
    spec = build_spec(cfg)
    nso = spec_json()['cfgs'][cfg]['n_solved']
    if not nso:
        return 0
    be = backend_cls(spec, nso, **kw)
    lens = [len(g['so%d_action' % k]) for k in range(nso)]
    exp_map = np.stack([g['so%d_map0' % k] for k in range(nso)])
    for k in range(nso):
        be.load(k, g['so%d_map0' % k], g['so%d_loc0' % k], g['so%d_facing0' % k],
                inv=g['so%d_inv0' % k] if 'so%d_inv0' % k in g else None)
    md = [{} for _ in range(nso)]
    for k in range(nso):
        for t, i, v in zip(g['so%d_md_t' % k], g['so%d_md_i' % k], g['so%d_md_v' % k]):
            md[k].setdefault(int(t), []).append((int(i), int(v)))
    for t in range(max(lens)):
        acts = np.array([g['so%d_action' % k][t] if t < lens[k] else 1 for k in range(nso)], np.int32)
        out = be.step(acts)
        st = be.state()
        for k in range(nso):
            if t >= lens[k]:
                continue
            p = 'so%d_' % k
            where = '%s solved %d step %d' % (cfg, k, t)
            check_outs(spec, out, k, acts[k], g[p + 'reward'][t], g[p + 'done'][t], g[p + 'result'][t], g[p + 'cost'][t],
                       g[p + 'cost_is_int'][t], g[p + 'msg'][t], where)
            for i, v in md[k].get(t, ()):
                exp_map[k, i] = v
            assert (st['loc'][k] == g[p + 'loc'][t]).all() and st['facing'][k] == g[p + 'facing'][t], where
            assert st['sel'][k] == g[p + 'sel'][t] and (st['inv'][k] == g[p + 'inv'][t]).all(), where
            assert (st['map'][k] == exp_map[k]).all(), where
        for k in range(nso):
            if t == lens[k] - 1:
                assert g['so%d_done' % k][t] == 1
    return sum(lens)


class HipBackend:
    """n envs on the MI355X through the C-ABI (VecNovelGridworld); same interface as OracleBackend."""

    def __init__(self, spec, n, **kw):
        from gym_novel_gridworlds_amd import VecNovelGridworld
        self.spec = spec
        self.v = VecNovelGridworld(spec=spec, num_envs=n, **kw)
        self.n = n

    def load(self, i, map_, loc, facing, inv=None, sel=0, step_count=0):
        K = self.v.n_items
        self.v.set_state(i, map=np.asarray(map_, np.int8)[None], loc=np.asarray(loc, np.int32)[None],
                         facing=np.array([facing], np.int32),
                         inv=np.zeros((1, K), np.int32) if inv is None else np.asarray(inv, np.int32)[None],
                         selected=np.array([sel], np.int32), step_count=np.array([step_count], np.int32))

    def load_all(self, map_, loc, facing, inv, sel):
        self.v.set_state(0, map=map_, loc=loc, facing=facing, inv=inv, selected=sel,
                         step_count=np.zeros(self.n, np.int32))

    def add_inventory(self, i, item, q):
        st = self.v.get_state(i, 1)
        st['inv'][0, item] += q
        self.v.set_state(i, inv=st['inv'])

    def step(self, actions):
        import ctypes as C
        from gym_novel_gridworlds_amd import _cabi
        a = np.ascontiguousarray(actions, np.int32)
        L = _cabi.lib()
        rc = L.ngw_step(self.v._h, _cabi._ptr(a, np.int32))
        if rc == _cabi.E_INVALID_ACTION:
            return dict(flags=1)
        _cabi.check(rc)
        reward, done, info = self.v.get_step_out(copy=True)
        return dict(flags=self.v.error_flags(), reward=reward, done=done.astype(np.uint8), result=info['result'].astype(np.uint8),
                    cost_code=info['step_cost_code'], msg_code=info['message_code'], msg_arg=info['message_arg'])

    def state(self):
        st = self.v.get_state()
        return dict(map=st['map'], loc=st['loc'], facing=st['facing'], inv=st['inv'], sel=st['selected'],
                    step_count=st['step_count'], episode=st['episode'])


class OracleVec:
    """Stand-in for VecNovelGridworld(num_envs=n) on the CPU oracle: the subset of the interface the single-env
    adapter (gym_novel_gridworlds_amd/envs.py) uses.  Lets the adapter's HOST logic run in the CPU-only suite."""

    def __init__(self, spec, num_envs=1, seed=0, autoreset=False, horizon=0, env_index_base=0, **_):
        from oracle.ngw_oracle import Oracle
        self.spec, self.num_envs = spec, num_envs
        self.o = Oracle(spec.compile(), num_envs, seed=seed, env_index_base=env_index_base, autoreset=autoreset, horizon=horizon)

    def reset(self, mask=None, copy=False):
        from gym_novel_gridworlds_amd.vec_env import PLACEMENT_MESSAGE
        if self.o.reset(mask) & 2:
            raise AssertionError(PLACEMENT_MESSAGE)

    def step(self, actions, copy=False):
        a = np.ascontiguousarray(actions, np.int32)
        A = len(self.spec.actions_id)
        for x in a:
            if x < 0 or x >= A:
                raise ValueError("%d is not in list" % x)
        self.o.step(a)
        o = self.o
        info = {'result': o.result.astype(bool), 'step_cost_code': o.cost_code, 'message_code': o.msg_code, 'message_arg': o.msg_arg}
        return None, o.reward.copy(), o.done.astype(bool), info

    # the one-env entry points the gym.Env adapter drives (VecNovelGridworld.reset1 / step1 / last_state)
    def reset1(self):
        self.reset()

    def step1(self, action):
        _, reward, done, info = self.step(np.array([action], np.int32))
        return (int(reward[0]), bool(done[0]), bool(info['result'][0]), int(info['step_cost_code'][0]), int(info['message_code'][0]),
                int(info['message_arg'][0]))

    def last_state(self):
        st = self.o.st
        return dict(map=st.map, loc=st.loc, facing=st.facing, inv=st.inv, selected=st.selected, step_count=st.step_count)

    def last_state1(self):
        st = self.o.st
        return (np.ascontiguousarray(st.map[0], np.int8).tobytes(), int(st.loc[0][0]), int(st.loc[0][1]), int(st.facing[0]),
                np.ascontiguousarray(st.inv[0], np.int32).tobytes(), int(st.selected[0]), int(st.step_count[0]))

    def get_state(self, first=0, count=None):
        st = self.o.st
        count = self.num_envs - first if count is None else count
        sl = slice(first, first + count)
        return dict(map=st.map[sl].copy(), loc=st.loc[sl].copy(), facing=st.facing[sl].copy(), inv=st.inv[sl].copy(),
                    selected=st.selected[sl].copy(), step_count=st.step_count[sl].copy(), episode=st.episode[sl].copy())

    def set_state(self, first=0, map=None, loc=None, facing=None, inv=None, selected=None, step_count=None, episode=None):
        st = self.o.st
        for arr, dst in ((map, st.map), (loc, st.loc), (facing, st.facing), (inv, st.inv), (selected, st.selected),
                         (step_count, st.step_count), (episode, st.episode)):
            if arr is not None:
                arr = np.asarray(arr)
                dst[first:first + len(arr)] = arr.reshape((len(arr),) + dst.shape[1:])

    def close(self):
        pass

    def sync(self):
        pass

    def rebuild(self, spec):
        """inject_novelty on the stand-in: the same env (seed, global env indices, settings) on the edited spec."""
        from oracle.ngw_oracle import Oracle
        o = self.o
        self.spec = spec
        self.o = Oracle(spec.compile(), self.num_envs, seed=o.seed, env_index_base=o.base, autoreset=o.autoreset, horizon=o.horizon)
        return self

    def lidar_configure(self, lidar_config=None, num_beams=8, fused=False, dtype=None):
        from gym_novel_gridworlds_amd.lidar import LidarConfig
        self.lidar = lidar_config if lidar_config is not None else LidarConfig(self.spec, num_beams)
        self._lidar_c = self.lidar.compile(self.spec)

    def agent_view(self, view_size=5, device=False, copy=False):
        from oracle.ngw_oracle import agent_view
        return agent_view(self.o.st.map, self.o.st.loc, view_size)

    def lidar_observation(self, device=False, copy=False):
        from oracle.ngw_oracle import lidar
        st = self.o.st
        return lidar(self._lidar_c, self.spec.map_size, len(self.spec.items_id), st.map, st.loc, st.facing, st.inv)

    def device_observation(self):
        import torch
        st, S = self.o.st, self.spec.map_size
        return {'map': torch.from_numpy(st.map).reshape(-1, S, S), 'agent_location': torch.from_numpy(st.loc),
                'agent_facing_id': torch.from_numpy(st.facing), 'inventory_items_quantity': torch.from_numpy(st.inv)}

    def device_outputs(self):
        import torch
        return {'reward': torch.from_numpy(self.o.reward), 'done': torch.from_numpy(self.o.done),
                'info': torch.from_numpy(self.o.info.view(np.int32))}


def make_adapter_env(cfg, backend='hip', seed=5):
    """Single-env adapter for a fixture configuration, built the way a reference user would build it."""
    import gym_novel_gridworlds_amd as G
    env_id, S, nov = CFGS[cfg]
    env = G.make(env_id)
    if backend == 'oracle':
        env._make_backend = lambda spec, seed_: OracleVec(spec, 1, seed=seed_)
    env.seed(seed)
    env.map_size = S
    if nov is not None:
        if cfg in REMAP_SEED:
            np.random.seed(REMAP_SEED[cfg])
        for one in novelty_list(nov):
            env = G.inject_novelty(env, *one)
    return env


def adapter_inject(base, spec, m, loc, facing, sel, inv):
    """State injection by direct attribute mutation, like the reference's users (keyboard_interface.py:93-100)."""
    S = base.map_size
    names = spec.item_names
    base.map[...] = np.asarray(m).reshape(S, S)
    base.agent_location = (int(loc[0]), int(loc[1]))
    base.set_agent_facing(['NORTH', 'SOUTH', 'WEST', 'EAST'][int(facing)])
    base.inventory_items_quantity = {names[i]: int(inv[i]) for i in range(len(inv))}
    base.selected_item = names[int(sel)] if sel else ''
    base.update_block_in_front()


def replay_adapter(cfg, backend, max_steps=400, n_single=300):
    """Golden traces + single steps through the reference-shaped API: Dict obs, python reward/done, info dict."""
    g = golden(cfg)
    env = make_adapter_env(cfg, backend)
    base = env.unwrapped if hasattr(env, 'unwrapped') else env
    spec = base._spec
    env.reset()
    K = len(spec.items_id)
    names = spec.item_names
    checked = 0
    p = 'tr0_'
    rl = {int(t): j for j, t in enumerate(g[p + 'rl_t'])}
    inj = {}
    for t, it, q in zip(g[p + 'inj_t'], g[p + 'inj_item'], g[p + 'inj_q']):
        inj.setdefault(int(t), []).append((int(it), int(q)))
    for t in range(min(max_steps, len(g[p + 'action']))):
        if t in rl:
            j = rl[t]
            adapter_inject(base, spec, g[p + 'rl_map'][j], g[p + 'rl_loc'][j], g[p + 'rl_facing'][j], 0,
                           g[p + 'rl_inv'][j] if p + 'rl_inv' in g else np.zeros(K, int))
            base.step_count = 0
        for it, q in inj.get(t, ()):
            base.inventory_items_quantity[names[it]] += q
        a = int(g[p + 'action'][t])
        obs, reward, done, info = env.step(a)
        exp_cost = g[p + 'cost'][t]
        assert type(reward) is int and reward == g[p + 'reward'][t] and type(done) is bool and done == bool(g[p + 'done'][t]), (cfg, t)
        assert info['result'] is bool(g[p + 'result'][t]) and info['message'] == messages()[g[p + 'msg'][t]], (cfg, t, info)
        assert info['step_cost'] == exp_cost and (type(info['step_cost']) is int) == bool(g[p + 'cost_is_int'][t]), (cfg, t)
        assert obs['agent_location'] == tuple(g[p + 'loc'][t]) and obs['agent_facing_id'] == g[p + 'facing'][t]
        assert obs['map'] is base.map and obs['inventory_items_quantity'] is base.inventory_items_quantity
        assert [obs['inventory_items_quantity'][n] for n in names] == list(g[p + 'inv'][t])
        assert (base.selected_item or '') == (names[g[p + 'sel'][t]] if g[p + 'sel'][t] else '')
        assert cfg.startswith('stk_') or base.step_count == g[p + 'step_count'][t]
        checked += 1
    exp_map = g['ss_pre_map'].copy()
    exp_map[g['ss_md_c'], g['ss_md_i']] = g['ss_md_v']
    for c in range(min(n_single, len(g['ss_action']))):
        adapter_inject(base, spec, g['ss_pre_map'][c], g['ss_pre_loc'][c], g['ss_pre_facing'][c], g['ss_pre_sel'][c], g['ss_pre_inv'][c])
        obs, reward, done, info = env.step(int(g['ss_action'][c]))
        assert reward == g['ss_reward'][c] and done == bool(g['ss_done'][c]) and info['message'] == messages()[g['ss_msg'][c]], (cfg, c)
        assert (np.asarray(obs['map']).ravel() == exp_map[c]).all() and base.block_in_front_id == base.map[base.block_in_front_location]
        checked += 1
    env.close()
    return checked


# ---------------------------------------------------------------- G6: distribution of the reset passes (tests/golden/gen_g6.py)
G6_CFGS = ('add32', 'add12m', 'add11e', 'crate12h', 'fire14m', 'fire10h', 'replwall12e')


def g6_stats(maps, locs, item, S):
    """What gen_g6.py records for the reference, for a batch of freshly reset envs: per-cell frequency of the pass item,
    histogram of the number of such cells per env, per-cell frequency of the agent cell."""
    m = np.asarray(maps).reshape(len(maps), S * S) == item
    freq = m.sum(0).astype(np.int64)
    hist = np.bincount(m.sum(1), minlength=S * S + 1).astype(np.int64)
    agent = np.bincount(np.asarray(locs)[:, 0].astype(np.int64) * S + np.asarray(locs)[:, 1], minlength=S * S).astype(np.int64)
    return freq, hist, agent


def _two_sample_z2(a, na, b, nb):
    """Sum of squared z-scores of two binomial samples per bin (pooled variance) and the number of bins that can differ."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = (a + b) / (na + nb)
    var = p * (1 - p) * (1.0 / na + 1.0 / nb)
    use = var > 0
    z2 = ((a[use] / na - b[use] / nb) ** 2 / var[use]).sum()
    # bins where both samples agree exactly on "never" / "always" carry no information; they must agree, though
    assert ((a[~use] == 0) == (b[~use] == 0)).all(), "a cell the reference never / always fills differs"
    return float(z2), int(use.sum())


def g6_check(cfg, freq, hist, agent, n):
    """Two-sample chi-square of a batch's statistics against the reference's (tests/golden/g6_<cfg>.npz).  The sum of k
    squared z-scores has mean k and standard deviation ~sqrt(2k): six of those is the bound (seeds are fixed, so a pass
    stays a pass)."""
    g = dict(np.load(os.path.join(GOLDEN, 'g6_%s.npz' % cfg)))
    na = int(g['n'])
    for name, a, b in (('item cells', g['freq'], freq), ('agent cell', g['agent'], agent)):
        z2, k = _two_sample_z2(a, na, b, n)
        assert z2 < k + 6 * (2 * k) ** 0.5 + 10, "%s: %s frequencies differ from the reference (chi2 %.1f over %d cells)" % (cfg, name, z2, k)
    # count histogram: merge bins until each holds >= 20 reference resets
    ha, hb = g['hist'].astype(np.int64), np.asarray(hist, np.int64)
    assert ha.sum() == na and hb.sum() == n
    nz = np.nonzero(ha + hb)[0]
    A, B, ca, cb = [], [], 0, 0
    for i in nz:
        ca += ha[i]; cb += hb[i]
        if ca >= 20:
            A.append(ca); B.append(cb); ca = cb = 0
    if A:
        A[-1] += ca; B[-1] += cb
    else:
        A, B = [ca], [cb]
    if len(A) > 1:
        z2, k = _two_sample_z2(A, na, B, n)
        assert z2 < k + 6 * (2 * k) ** 0.5 + 10, "%s: count histogram differs from the reference (chi2 %.1f over %d bins)" % (cfg, z2, k)
    else:
        assert np.nonzero(ha)[0].tolist() == np.nonzero(hb)[0].tolist(), "%s: the count is a constant in the reference" % cfg
    mean_a, mean_b = (ha * np.arange(len(ha))).sum() / na, (hb * np.arange(len(hb))).sum() / n
    return mean_a, mean_b


def oracle_sharded(**kw):
    """ShardedVecNovelGridworld whose local envs run on the CPU oracle (CPU-only suite: gloo ranks, no GPU): the product class
    with its three device hooks replaced - the local env, the payload pack and the unpack - by host code over the same bytes."""
    import torch
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld

    class OracleSharded(ShardedVecNovelGridworld):
        def _make_local(self, device=None, spec=None, **k):
            k = {a: b for a, b in k.items() if a in ('num_envs', 'seed', 'autoreset', 'horizon', 'env_index_base')}
            return OracleVec(spec, **k)

        def payload_layout(self):
            n, S, K = self.num_envs, self.spec.map_size, len(self.spec.items_id)
            offs = [0]
            for w in (S * S, 8, 4, 4 * K, 4, 1, 4):
                offs.append(offs[-1] + ((n * w + 15) & ~15))
            return offs

        def packed_observation(self):
            offs = self.payload_layout()
            o, out = self.local.device_observation(), self.local.device_outputs()
            buf = torch.zeros(offs[7], dtype=torch.uint8)
            parts = [o['map'], o['agent_location'], o['agent_facing_id'], o['inventory_items_quantity'], out['reward'], out['done'], out['info']]
            for off, t in zip(offs, parts):
                b = t.contiguous().reshape(-1).view(torch.uint8)
                buf[off:off + b.numel()] = b
            return buf

        def unpack(self, payloads, world=None):
            world = self.world if world is None else world
            n, offs = self.num_envs, self.payload_layout()
            pl = payloads.reshape(world, offs[7])
            out = {}
            for name, off, (sh, dt), (sh1, _) in zip(self.FIELDS, offs, self._field_shapes(n * world), self._field_shapes(n)):
                nbytes = int(torch.tensor([], dtype=dt).element_size())
                for d in sh1:
                    nbytes *= d
                out[name] = pl[:, off:off + nbytes].contiguous().view(dt).reshape(sh)
            out['done'] = out['done'].bool()
            return out

    return OracleSharded(**kw)


def info_word(o):
    """uint32 [n]: the packed info word of the oracle's last step - result | goal_done << 1 | cost_code << 2 | msg_code << 8 | msg_arg << 16."""
    goal_done = (o.info >> np.uint32(1)) & np.uint32(1)
    return (o.result.astype(np.uint32) | (goal_done << np.uint32(1)) | (o.cost_code.astype(np.uint32) << np.uint32(2)) |
            (o.msg_code.astype(np.uint32) << np.uint32(8)) | (o.msg_arg.astype(np.uint32) << np.uint32(16)))


def sharded_on_oracle(cls, **kw):
    """The product's ShardedVecNovelGridworld with its local env replaced by the oracle-backed stand-in `cls` (no GPU)."""
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld

    class OracleSharded(ShardedVecNovelGridworld):
        def _make_local(self, device=None, spec=None, **k):
            k = {a: b for a, b in k.items() if a in ('num_envs', 'seed', 'autoreset', 'horizon', 'env_index_base')}
            return cls(spec, **k)

    return OracleSharded(**kw)
