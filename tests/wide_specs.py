"""The wide specs: legal specs at and near the limits of the ABI - NGW_MAX_ITEMS = 24, NGW_MAX_ACTIONS = 48, NGW_MAX_RECIPES = 8 - built
through the public EnvSpec surface from ngw_testlib.build_spec bases (add_new_item + add_select_action, new entries of `recipes` with
their Craft_* ids, Jump / Chop, max_items raised for K > 20 only).  tests/test_wide_specs_cpu.py holds every row to this table and shows on
the CPU oracle that the wide columns are part of play; tests/test_wide_specs.py runs the device against the oracle on them.

    name      K   A   R  entities  S   base             step kernel  what it pins
    p12a34    12  34  8  0         10  pogo10           plain        bits >= 32 in the plain-step specialisation (K <= 12 is its bound)
    w20       20  31  7  0         10  pogo10           general      the reference's own limit of 20 items, A <= 32
    w20a33    20  33  8  0         10  bow10            general      one action in the third slot of 16 / bit 32, a Jump and a Chop
    w21       21  30  5  0         12  jump12           general      the first K past the reference's cap, odd, 16-byte maps
    w24       24  38  8  1         10  stk_fire_axeh10  extended     the item limit, 8 recipes, an entity and a FireWall
    w24a48    24  48  8  1         12  stk_fire_axeh10  extended     both limits: 10 alias actions behind the 38 named ones

"plain" is ngw_step_lean<..., PLAIN> (no Jump, no entity, K <= 12: ngwh_step_plain_class), "general" the same kernel's general
instantiation, "extended" the instantiation with the wrapper predicates (FireWall here).  No spec with K > 12 can be plain, so the plain
row is wide in A alone.

The added items are breakable, some lie on the map (items_quantity), some start in the inventory (start_inventory); the item with id
K - 1 ('zinc') comes out of a one-input recipe whose input starts in the inventory, the goal's recipe consumes it, and the recipe named
last - index R - 1, 7 where R = 8 - is that recipe.  Every added item is a lidar item of a LidarConfig made from the grown spec."""
import copy
import functools

import numpy as np

import expand_oracle as XO
import ngw_testlib as T
import snapshot_oracle as SO
from gym_novel_gridworlds_amd.spec import EnvSpec

NAMES = ('amber', 'basalt', 'clay', 'dune', 'ember', 'flint', 'gravel', 'hemp', 'ivory', 'jade', 'kelp', 'lime')
LAST = 'zinc'
# name: (K, A, R, n_entities, S, base, step kernel)
TABLE = {
    'p12a34': (12, 34, 8, 0, 10, 'pogo10', 'plain'),
    'w20': (20, 31, 7, 0, 10, 'pogo10', 'general'),
    'w20a33': (20, 33, 8, 0, 10, 'bow10', 'general'),
    'w21': (21, 30, 5, 0, 12, 'jump12', 'general'),
    'w24': (24, 38, 8, 1, 10, 'stk_fire_axeh10', 'extended'),
    'w24a48': (24, 48, 8, 1, 12, 'stk_fire_axeh10', 'extended'),
}
ALL = tuple(TABLE)
WIDE_A = tuple(n for n in ALL if TABLE[n][1] > 32)
N_ENVS, N_PAIRS, STEPS, KEYS, WARM = 65, 130, 8, 4096, 24


class AliasSpec(EnvSpec):
    """An EnvSpec with alias actions: `aliases` maps a new action name to the name of an earlier action whose kind and argument it repeats.
    The alias names are in actions_id (VecNovelGridworld.n_actions is len(actions_id)); compile() lets the parent flatten the named actions
    and fills act_kind / act_arg of the aliases behind them."""

    @classmethod
    def of(cls, base):
        spec = cls.__new__(cls)
        spec.__dict__.update(copy.deepcopy(base.__dict__))
        spec.aliases = {}
        return spec

    def add_alias(self, name):
        alias = '%s_%d' % (name, len(self.actions_id))
        self.aliases[alias] = name
        self.actions_id[alias] = len(self.actions_id)

    def compile(self):
        self.validate()                                                              # (with the aliases counted)
        full = self.actions_id
        self.actions_id = {n: a for n, a in full.items() if n not in self.aliases}
        try:
            s = EnvSpec.compile(self)
        finally:
            self.actions_id = full
        s.n_actions = len(full)
        for alias, name in self.aliases.items():
            s.act_kind[full[alias]], s.act_arg[full[alias]] = s.act_kind[full[name]], s.act_arg[full[name]]
        return s


def add_manipulation(spec, name):
    spec.manipulation_actions_id[name] = len(spec.actions_id)
    spec.actions_id.update(spec.manipulation_actions_id)
    spec.action_space_n = len(spec.actions_id)


def add_recipe(spec, out, inputs, qty, costs=(0, 0, 2400.0)):
    spec.recipes[out] = {'input': dict(inputs), 'output': {out: qty}}
    spec.craft_costs[out] = costs
    spec.craft_actions_id['Craft_' + out] = len(spec.actions_id)
    spec.actions_id.update(spec.craft_actions_id)


def grow(base, n_items, n_recipes, manipulation=(), max_items=None, map_size=None, on_map=(2, 2, 1)):
    """The base spec with n_items added items (the last one LAST), their Select actions, n_recipes of the added recipes in the order below
    (LAST's recipe is the last action added), the named manipulation actions, and the added items in play."""
    spec = AliasSpec.of(T.build_spec(base, map_size=map_size))
    if max_items is not None:
        spec.max_items = max_items
    x = list(NAMES[:n_items - 1]) + [LAST]
    for name in manipulation:
        if name not in spec.actions_id:
            add_manipulation(spec, name)
    for name in x:
        spec.add_new_item(name)
        spec.add_select_action(name)
    # the inputs by position among the added items; x[3] (id >= 12 on every base) starts in the inventory
    feed, ore, mid = x[min(3, n_items - 2)], x[min(5, n_items - 2)], x[min(6, n_items - 2)]
    recipes = [(x[min(4, n_items - 2)], {LAST: 1, ore: 1}, 1, (360.0, 720.0, 7200.0)),
               (x[min(8, n_items - 2)], {'tree_log': 1, feed: 1}, 3, (0, 0, 1200.0)),
               (feed, {mid: 1, 'plank': 1}, 2, (480.0, 840.0, 8400.0)),
               (mid, {ore: 2}, 1, (0, 0, 2400.0)),
               (LAST, {feed: 1}, 2, (0, 0, 1200.0))]
    for out, inputs, qty, costs in recipes[len(recipes) - n_recipes:]:
        add_recipe(spec, out, inputs, qty, costs)
    spec.recipes[spec.goal_item_to_craft]['input'][LAST] = 1                         # the goal's demand reaches the added rules
    spec.items_quantity.update({name: q for name, q in zip((x[0], ore, x[-2]), on_map) if q})
    spec.start_inventory.update({feed: 5, ore: 2, x[-2]: 1})
    return spec


@functools.lru_cache(maxsize=None)
def spec_of(name):
    if name == 'p12a34':                                                             # 3 items and 4 recipes of its own: ids stop at 11
        spec = grow('pogo10', 3, 0)
        add_recipe(spec, 'crafting_table', {'plank': 4}, 1, (0, 0, 2400.0))
        add_recipe(spec, 'amber', {'tree_log': 1}, 2, (0, 0, 1200.0))
        add_recipe(spec, 'basalt', {'amber': 2, 'plank': 1}, 1, (360.0, 720.0, 7200.0))
        add_recipe(spec, LAST, {'basalt': 1}, 2, (0, 0, 1200.0))
        for i in range(10):
            spec.add_alias(('Select_zinc', 'Craft_zinc', 'Forward', 'Select_basalt', 'Left')[i % 5])
    elif name == 'w20':
        spec = grow('pogo10', 11, 3)
    elif name == 'w20a33':
        spec = grow('bow10', 11, 5, ('Jump', 'Chop'))
    elif name == 'w21':
        spec = grow('jump12', 12, 2, max_items=24)
    elif name == 'w24':
        spec = grow('stk_fire_axeh10', 13, 3, ('Jump', 'Chop'), max_items=24, on_map=(1, 0, 0))     # (a FireWall map of 10 x 10 has room for no more)
    elif name == 'w24a48':
        spec = grow('stk_fire_axeh10', 13, 3, ('Jump', 'Chop'), max_items=24, map_size=12)
        for i in range(10):
            spec.add_alias(('Select_zinc', 'Craft_zinc', 'Forward', 'Select_lime', 'Right', 'Select_dune', 'Craft_dune', 'Left', 'Select_flint', 'Break')[i])
    elif name == 'w24e':                                                             # w24a48 with entities and a break reward at ids >= 16
        spec = copy.deepcopy(spec_of('w24a48'))
        spec.entities |= {'jade', 'lime'}
        spec.break_reward_items.append('kelp')
    else:
        raise KeyError(name)
    return spec


def step_kernel_of(cs):
    """Which instantiation of the step kernel a compiled spec lands in, by the rules of csrc/ngw_abi_create.cpp."""
    from gym_novel_gridworlds_amd.spec import ACT_JUMP
    if cs.fire_item or cs.fence_mode or cs.crate_item:
        return 'extended'
    jump = any(int(cs.act_kind[a]) == ACT_JUMP for a in range(int(cs.n_actions)))
    return 'plain' if int(cs.n_items) <= 12 and not jump and not int(cs.n_entities) else 'general'


def mixed_actions(spec, st, rs):
    """One action per env: the even envs uniform over A, the odd ones uniform over the oracle's valid set (so wide actions succeed)."""
    import mask_oracle as M
    A = len(spec.actions_id)
    words = M.oracle_mask_words(spec, st)
    a = rs.randint(0, A, st.n).astype(np.int32)
    for i in range(1, st.n, 2):
        valid = [b for b in range(A) if (int(words[i]) >> b) & 1]
        if valid:
            a[i] = valid[rs.randint(len(valid))]
    return a, words


def rich_inventories(spec, st, rs):
    """Every third env of the dict `st` gets 0 to 5 of every breakable item: states with more than 32 valid actions."""
    cs = spec.compile()
    inv = np.array(st['inv'], np.int32).reshape(len(st['facing']), -1)
    for i in range(2, len(inv), 3):
        inv[i] = rs.randint(0, 6, inv.shape[1]) * np.array([int(cs.breakable[k]) for k in range(inv.shape[1])])
    return dict(st, inv=inv.reshape(np.asarray(st['inv']).shape))


@functools.lru_cache(maxsize=None)
def oracle_env(name, n=N_ENVS, warm=WARM):
    """-> (spec, seed, the start states - a reset, then rich_inventories -, the warm-up actions [warm, n], the oracle after them, and per
    warm-up step (mask words, the state before, results, message codes, message arguments))."""
    from oracle.ngw_oracle import Oracle
    spec = spec_of(name)
    seed = XO.good_seed(spec, n)
    o = Oracle(spec.compile(), n, seed=seed)
    o.reset()
    rs, acts, log = np.random.RandomState(len(name) + 40), [], []
    start = rich_inventories(spec, SO.oracle_state(o), rs)
    SO.put_state(o, start)
    for _ in range(warm):
        before = SO.oracle_state(o)
        a, words = mixed_actions(spec, o.st, rs)
        o.step(a)
        acts.append(a)
        log.append((words, before, np.asarray(o.result).astype(bool).copy(), o.msg_code.copy(), o.msg_arg.copy()))
    return spec, seed, start, np.stack(acts), o, log


def rows_of(name):
    """The 65 states after the warm-up, as a dict keyed like get_state()."""
    return SO.oracle_state(oracle_env(name)[4])


def wide_crafted_rows(A):
    """test_tree_rule_cpu.crafted_rows(A) and, behind them, the rows of the three slots of 16 lanes (A > 32)
    -> (visits, returns, masks, priors, names)."""
    import test_tree_rule_cpu as XR
    v0, r0, m0, p0, names = XR.crafted_rows(A)
    n, full, hi = 10, (1 << A) - 1, ((1 << A) - 1) & ~((1 << 32) - 1)
    v, r, m, p = np.ones((n, A), np.int32), np.full((n, A), -50, np.int64), np.full(n, full, np.uint64), np.ones((n, A), np.float32)
    more = ['a winner in slot 0', 'a winner in slot 1', 'a winner in slot 2', 'equal best at 0, 16 and 32', 'equal best at two lanes of slot 2', 'only bits >= 32',
            'the lowest bit is 32, unvisited there, a better mean at A - 1', 'bits at and above A', 'bits above A alone beside bit 33 % A', 'all A valid, nothing visited']
    r[0, 5], r[1, 21], r[2, A - 1] = 100, 100, 100
    r[3, [0, 16, 32]] = 0
    r[4, [32, A - 1]] = 0                                                            # (A = 33: one lane - a unique winner there)
    m[5] = hi
    m[6], v[6, 32], r[6, 32], r[6, A - 1] = hi, 0, 0, 70                             # (q_init or NaN at 32 against + 70 at A - 1)
    p[6, 32] = np.nan                                                                # (a NaN prior there: clamped to 0, F_BAD_WEIGHT)
    if A < 64:
        m[7] = np.uint64(full | (0xFFFF << A) & 0xFFFFFFFFFFFFFFFF)
        m[8] = np.uint64((1 << (33 % A)) | (0xFFFF << A) & 0xFFFFFFFFFFFFFFFF)
    v[9], r[9] = 0, 0
    return np.concatenate([v0, v]), np.concatenate([r0, r]), np.concatenate([m0, m]), np.concatenate([p0, p]), names + more
