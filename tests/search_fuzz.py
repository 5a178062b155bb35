"""Model-based fuzz of the whole search surface of one handle: the driver and the model (tests/test_search_fuzz.py runs it against the HIP
path, tests/test_search_fuzz_cpu.py against an oracle-backed stand-in and against seeded faults).

run_case() draws the handle's settings and 8 - 15 calls - writers of live state, writers of snapshot slots, read-only calls - performs each on the
env under test and on the model, and compares after EVERY call: the seven state arrays, every open snapshot, the call's own return value, the
fused lidar rows, the action-mask words, the terminal-observation rows and the error flags.  The model is the CPU oracle for the live envs,
snapshot_oracle.NumpySnapshot for the slots, key_table_oracle.KeyTableModel for the tables and the row-level reference functions of
tests/*_oracle.py for everything a call returns; nothing in it calls the HIP library or the package's own host restatements of the contracts
(path keys are hashed here from the rows path_key_oracle hands back, by state_key_oracle's rule).  The one exception is the guided playout, whose
reference - guided_playout_oracle.oracle_guided - is built on the public numpy contracts of the Philox word, the weighted choice and the key.

The two newest features are forms and kinds of their own.  'view': a trajectory call with observe='agent_view' and a drawn view_size, on rollout,
playout and playouts, held to trajectory_view_oracle.expect_views.  'splayout_guided' / 'splayout_guided_kids' and the 'guided' form of playouts: a
guided playout over the case's ONE key table - whatever insert_state_keys, insert_succ_keys, slot_insert_keys and table_insert put there, under
whatever fields, plus (three times in four) an offer of keys under the call's own fields - with limits, outside='stop', first_pair up to 2^40, every
source, children, every fields choice, both observations.  table_weights holds f(key) in the bucket the table REPORTED for each key the model holds
and NaN in every other row, so a lane that reads a bucket no member owns changes the actions or raises F_BAD_WEIGHT, which check_all holds to 0.
FIELD_CHOICES includes KEY_INV alone: with an empty inventory that key is 0, the one key a table never stores and a guided step never looks up.

Walks, frontiers and the skipped pair.  Any call drawn in its device form whose index lists live on the device may be PADDED (draw_pad, one time in
two): a scattered third, entries 64 .. 127 of a list longer than 128, all but one or all of its entries become IDX_NONE - in the source list, the
destination list or both.  The references run on the list as drawn (the pairs of one call do not see each other), and the pairs that are not there get
what include/ngw.h says the call stores for them: nothing, zeros, action -1, key 0, distance -1, where -1 and fresh 0 at the table; their destination
rows are not written in the model, so check_all holds them byte-identical, and F_BAD_INDEX stays 0.  'slot_walk' / 'walk': walk_distances and
walk_plans of filled slots and of the live envs against walk_oracle, every item id, 1 - 12 steps.  'walk_go': walk_plans(device=True) fed to
rollout(limits=length.clip(0, steps), children=) with nothing leaving the device.  'frontier_compact': Frontier.compact of drawn flag bytes, taken 0 -
15 bytes into a larger tensor, against frontier_oracle.  'frontier_step': insert_successor_keys -> fresh_pairs -> alloc -> expand on a padded parents
list, the cursor and limit drawn so that no slot handed out is a parent of the call.  F_FRONTIER_FULL is compared by the call that raises it
(error_flags reads and clears).  'frontier_twins': a device-form guided playout recorded with record=True, then fr.fresh_steps (of
the flags the table reports for its path keys), fr.transitions and fr.tree_steps against the same lists of the model's expected result, padded by
frontier_oracle, each at a capacity below, at and above the hits.

Every draw depends on the RandomState, the settings and the model alone - never on a value the env under test returned - and every draw of a call is
made before the model decides whether the call is refused, so the walk of a seed is the same walk on every backend.  The one state-dependent exit is
"Cannot place items": both sides must fail, and the case ends.

What the env under test must offer beyond VecNovelGridworld's own surface: to_device(numpy array) -> what the device-input forms take, and
ptr_of(that) -> what step_device_many / rollout_actions / graph_build take.  No GPU import at module level."""
import os

import numpy as np

import expand_oracle as XO
import frontier_oracle as FO
import guided_playout_oracle as GO
import key_table_oracle as KT
import lookahead_oracle as LO
import mask_oracle as M
import ngw_testlib as T
import path_key_oracle as KO
import plan_oracle as PL
import playout_oracle as PO
import sample_oracle as SA
import slot_observe_oracle as OO
import slot_rollout_oracle as RO
import snapshot_oracle as SO
import state_key_oracle as SK
import successor_key_oracle as SU
import trajectory_oracle as TO
import trajectory_view_oracle as VO
import walk_oracle as WO
from oracle import ngw_oracle as NO

STATE_KEYS = SO.STATE_KEYS
SUCC_MAX_MAP = 34                    # Snapshot.successor_keys: "Maps up to 34 x 34 ... beyond that the call raises" (MapsTooLarge)
MAX_PAIRS, MAX_STEPS, MAX_PLANS = 130, 8, 3
TABLE_CAPACITY = 4096                # 8192 buckets.  A condition, asserted after every insert: the model never holds more keys (a full table is not what
                                     # this fuzz models; a guided call's offer - up to 650 keys - is skipped on both sides where it would pass it).  The
                                     # committed walk's largest table holds 496 keys: sparse enough to stay cheap, dense enough for probe chains
VIEW_SIZES = (1, 2, 5, 6)
NONE = FO.IDX_NONE                   # include/ngw.h NGW_IDX_NONE: a pair that is not there
F_FRONTIER_FULL = FO.F_FRONTIER_FULL
WALK_STEPS = 12                      # walk plans of 1 .. 12 steps: complete ones and ones cut short
# The rows of one walk call: walk_oracle searches S x S x 4 poses per distinct row in Python, so beyond 16 x 16 a call walks few rows.  ngw_walk_launch
# (csrc/ngw_unit_walk.hip) starts one work-group per row - grid = count, one wavefront each -, so any call of two rows spans several work-groups.
WALK_ROWS_LARGE = 6
FRONTIER_TILE = 4096                 # csrc/ngw_device.h NGW_FRONTIER_TILE
FLAG_LENGTHS = (0, 1, 17, FRONTIER_TILE - 1, FRONTIER_TILE, FRONTIER_TILE + 1, 2 * FRONTIER_TILE + 17)
PAD_LAYOUTS = ('third', 'wave', 'but_one', 'all')      # the entries of a device list that become IDX_NONE: a scattered third, entries 64 .. 127 of a list
                                                       # longer than 128 (a shorter one: the third), all but one, all
PAD_ONE_IN = 2                                         # a call with device lists is padded one time in two (one in three left kinds of weight 2 unpadded)
PAD_SIDES = ('source', 'destination', 'both')        # where a pair is skipped (a call with one list: that list; a walk: the row, the item, both)
FIELD_CHOICES = (SK.STATE, SK.ALL, SK.MAP | SK.POSE, SK.INV | SK.SELECTED, SK.STEP_COUNT | SK.EPISODE | SK.POSE, SK.MAP, SK.INV)

# call kinds and how often each is drawn (tests/test_search_fuzz_cpu.py holds the coverage these give for the committed seed)
KINDS = {
    # writers of live state
    'step': 3, 'dev': 2, 'rollout': 2, 'rollact': 2, 'reset': 2, 'mask_reset': 2, 'state_steps': 2, 'state_rows': 2, 'step_sampled': 2,
    'restore': 4, 'fork': 2, 'graph_launch': 2,
    # writers of slots only
    'save': 2, 'copy': 2, 'expand': 4, 'expand_all': 2, 'srollout_kids': 6, 'splayout_kids': 7, 'splayout_guided_kids': 4, 'walk_go': 6,
    'frontier_step': 6,              # (and of the table)
    # read-only (a guided playout offers keys to the table first: the env and the slots stay as they are)
    'splayout_guided': 4,
    'mask_words': 2, 'lookahead': 2, 'plans': 2, 'state_keys': 2, 'succ_keys': 2, 'insert_state_keys': 2, 'insert_succ_keys': 2, 'table_insert': 2,
    'table_lookup': 2, 'sample': 2, 'playouts': 6, 'srollout': 6, 'splayout': 6, 'slot_lidar': 2, 'slot_view': 2, 'slot_masks': 2, 'slot_keys': 2,
    'slot_unique': 2, 'slot_insert_keys': 2, 'agent_view': 2, 'lidar': 2, 'slot_walk': 6, 'walk': 6, 'frontier_compact': 6, 'frontier_twins': 6,
}
READ_ONLY = ('mask_words', 'lookahead', 'plans', 'state_keys', 'succ_keys', 'insert_state_keys', 'insert_succ_keys', 'table_insert', 'table_lookup', 'sample',
             'playouts', 'srollout', 'splayout', 'splayout_guided', 'slot_lidar', 'slot_view', 'slot_masks', 'slot_keys', 'slot_unique', 'slot_insert_keys',
             'agent_view', 'lidar', 'slot_walk', 'walk', 'frontier_compact', 'frontier_twins')
ROLLOUT_FORMS = ('plain', 'path', 'traj', 'view')
PLAYOUT_FORMS = ('plain', 'weighted', 'path', 'traj', 'view')
PLAYOUTS_FORMS = ('plain', 'weights', 'path_keys', 'rewards', 'masks', 'observe', 'view', 'guided')
GUIDED_KINDS = ('splayout_guided', 'splayout_guided_kids')
OFFER_KEEP = (0.25, 0.6, 1.0)        # the share of the offered keys a guided call keeps (drawn per call): thin tables give the misses and re-entries


class Refused(Exception):
    """The model's prediction: the env under test must raise `error` (a class) for this call, and nothing may change."""

    def __init__(self, error):
        Exception.__init__(self, error.__name__)
        self.error = error


# ---------------------------------------------------------------- small helpers
def host(x):
    """A result of either kind (numpy / torch, a tuple of them, None) as numpy."""
    if x is None:
        return None
    if isinstance(x, tuple):
        return tuple(host(y) for y in x)
    return x if isinstance(x, np.ndarray) else (x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x))


def same_bits(g, e):
    """g seen in e's dtype where the two differ only in signedness / bool-ness (a tensor's int64 words are the host's uint64)."""
    g, e = np.asarray(g), np.asarray(e)
    if g.dtype != e.dtype:
        if g.dtype.kind in 'iu' and e.dtype.kind in 'iu' and g.dtype.itemsize == e.dtype.itemsize:
            g = np.ascontiguousarray(g).view(e.dtype)
        elif e.dtype == np.bool_:
            g = g.astype(np.bool_)
        else:
            g = g.astype(e.dtype)
    return g


def eq(name, g, e, where):
    assert (g is None) == (e is None), "%s: %s is %s" % (where, name, 'missing' if g is None else 'not expected')
    if e is None:
        return
    g = same_bits(host(g), e)
    e = np.asarray(e)
    assert g.shape == e.shape, "%s: %s shape %r expected %r" % (where, name, g.shape, e.shape)
    bad = np.argwhere(g != e)
    assert not len(bad), "%s: %s differs at %d of %d places, first %s: got %r expected %r" % (
        where, name, len(bad), e.size, tuple(bad[0]), g[tuple(bad[0])], e[tuple(bad[0])])


def fast_keys(rows, fields):
    """uint64 [n]: state_key_oracle.keys_of(rows, 0 .. n-1, fields), every distinct value of a field hashed once (successor_key_oracle)."""
    n = len(rows['facing'])
    key = np.zeros(n, np.uint64)
    if n:
        for bit in SK.SINGLE:
            if fields & bit:
                key = key ^ SU.single_field_keys(rows, bit)
    return key


def rows_of(src):
    """A dict of the seven arrays of an oracle State or a NumpySnapshot (views, not copies)."""
    return src.rows if isinstance(src, SO.NumpySnapshot) else {k: getattr(src, k) for k in STATE_KEYS}


def rows_at(src, idx):
    r = rows_of(src)
    idx = np.asarray(idx, np.int64)
    return {k: r[k][idx] for k in STATE_KEYS}


def ref_pairs(spec, rows, parents, kind, autoreset, horizon, plans=None, steps=None, seed=0, first_pair=0, weights=None, limits=None, path_keys=False,
              fields=SK.STATE, rewards=False, masks=False, lc=None, view_size=None):
    """What one rollout / playout call must return and leave, from the row-level references: -> dict(ends, rep, actions [T, count], keys, rewards,
    masks, obs); the last four None where the call does not ask for them.  plans [count, T] for kind 'rollout'; weights [A] or None, steps and
    seed for kind 'playout'; lc: the LidarConfig with observe='lidar'; view_size: the window of observe='agent_view' (obs is then
    trajectory_view_oracle.expect_views' dict)."""
    parents = np.asarray(parents, np.int64)
    if kind == 'playout':
        if weights is None:
            ends, rep, actions, _ = PO.oracle_playout(spec, rows, parents, steps, seed, first_pair, autoreset, horizon)
        else:
            ends, rep, actions, _ = SA.oracle_weighted_playout(spec, rows, parents, steps, seed, weights, first_pair, autoreset, horizon)
    else:
        plans = np.asarray(plans)
        actions, steps = np.ascontiguousarray(plans.T), plans.shape[1]
    out = dict(keys=None, rewards=None, masks=None, obs=None)
    traj = rewards or masks or lc is not None or view_size is not None
    if not (traj or limits is not None or path_keys):
        if kind == 'rollout':
            ends, rep, _ = RO.oracle_slot_rollout(spec, rows, parents, plans, autoreset, horizon)
    else:
        if traj:
            e = TO.oracle_traj(spec, rows, parents, actions, limits, autoreset, horizon, fields, lc)
            ends, rp, states = e['ends'], e['reports'], e['states']
            out.update(rewards=e['rewards'] if rewards else None, masks=e['masks'] if masks else None, obs=e['obs'])
            if view_size is not None:
                out['obs'] = VO.expect_views(spec, rows, parents, e, view_size)
        else:
            _, rp, ends, states, _ = KO.oracle_path(spec, rows, parents, actions, limits, autoreset, horizon, fields)
        if kind == 'playout':                            # a limited playout is the prefix of the unlimited one: the actions beyond it are -1
            actions = np.where(np.arange(steps)[:, None] < rp['length'][None, :], actions, -1).astype(np.int32)
            rep = dict(rp, first_action=actions[0].copy())
        else:
            rep = rp
        if path_keys:                                    # the key of every visited row, by state_key_oracle's rule
            keys = np.zeros((steps, len(parents)), np.uint64)
            at = sorted(states)
            if at:
                kk = fast_keys({k: np.stack([np.asarray(states[i][k]) for i in at]) for k in STATE_KEYS}, fields)
                for (t, j), v in zip(at, kk):
                    keys[t, j] = v
            out['keys'] = keys
    out.update(ends=ends, rep=rep, actions=np.asarray(actions, np.int32))
    return out


def check_pairs(got, exp, kind, record, where):
    """A PlanEval / RolloutPath / RolloutTraj / Playout / PlayoutPath / PlayoutTraj (any leading shape) against ref_pairs' dict."""
    steps = exp['actions'].shape[0]
    for k in ('ret', 'length', 'ended', 'info') + (('first_action',) if kind == 'playout' else ()):
        eq(k, host(getattr(got, k)).reshape(-1), exp['rep'][k], where)
    if kind == 'playout':
        eq('actions', None if got.actions is None else host(got.actions).reshape(steps, -1), exp['actions'] if record else None, where)
    for k in ('keys', 'rewards', 'masks'):
        g = getattr(got, k, None)
        eq(k, None if g is None else host(g).reshape(steps, -1), exp[k], where)
    g = getattr(got, 'obs', None)
    if isinstance(exp['obs'], dict):                      # (observe='agent_view': the pair axes of every value flattened to the reference's one)
        assert isinstance(g, dict), "%s: obs is %s, a dict of views expected" % (where, type(g).__name__)
        g = {k: x.reshape(x.shape[0], -1, *x.shape[x.ndim - (exp['obs'][k].ndim - 2):]) if k in exp['obs'] else x for k, x in VO.OO.host(g).items()}
        VO.assert_views(g, exp['obs'], where)
        return
    eq('obs', None if g is None else TO.widen(g).reshape(steps + 1, -1, exp['obs'].shape[-1] if exp['obs'] is not None else 1), exp['obs'], where)


def state_dict(st):
    return {k: getattr(st, k).copy() for k in STATE_KEYS}


def blank_pairs(exp, skip):
    """ref_pairs' dict with what include/ngw.h says a rollout / playout stores for a skipped pair in the places of the pairs in `skip` (bool [count]):
    the four reports 0 (a rollout leaves them untouched: the zeros they were allocated as), first action and the column of actions -1, keys 0, rewards
    and masks 0, every block of the observation - block 0 included - zeros, where -1 and depth 0.  The end rows are left: the caller writes the live."""
    if skip is None:
        return exp
    out = dict(exp)
    out['rep'] = {k: np.where(skip, np.full((), -1 if k == 'first_action' else 0, np.asarray(v).dtype), v) for k, v in exp['rep'].items()}
    out['actions'] = np.where(skip[None, :], -1, exp['actions']).astype(np.int32)
    for k in ('keys', 'rewards', 'masks'):
        if exp.get(k) is not None:
            out[k] = np.where(skip[None, :], np.zeros((), exp[k].dtype), exp[k])
    obs = exp.get('obs')
    if isinstance(obs, dict):
        out['obs'] = {k: zero_pairs(v, skip) for k, v in obs.items()}
    elif obs is not None:
        out['obs'] = zero_pairs(obs, skip)
    return out


def zero_pairs(x, skip):
    x = np.array(x)
    x[:, skip] = 0
    return x


def walk_ids(cs):
    """(forward, left, right): "the LOWEST action id whose act_kind is NGW_ACT_FORWARD, NGW_ACT_LEFT and NGW_ACT_RIGHT respectively" (kinds 0, 1, 2),
    None for a kind the action table lacks."""
    ids = [None, None, None]
    for a in range(cs.n_actions):
        k = int(cs.act_kind[a])
        if k < 3 and ids[k] is None:
            ids[k] = a
    return tuple(ids)


# ---------------------------------------------------------------- one case
class Case:
    """The env under test, the model and the bookkeeping of one case."""

    def __init__(self, rs, cfg, case, make_env, log):
        self.rs, self.cfg, self.case, self.log = rs, cfg, case, log or (lambda *a: None)
        spec = self.spec = T.build_spec(cfg)
        self.A, self.S, self.K = len(spec.actions_id), spec.map_size, len(spec.items_id)
        S = self.S
        n = self.n = int(rs.choice([1, 63, 64, 65, 130])) if S <= 16 else int(rs.choice([1, 64, 65]))
        self.horizon = int(rs.choice([0, 5, 23]))
        self.autoreset = bool(rs.randint(0, 4)) or self.horizon > 0
        prefetch = rs.choice(['auto', 0, 3])
        self.prefetch = prefetch if prefetch == 'auto' else int(prefetch)
        self.depth = int(rs.choice([0, 1, 2]))
        self.term = bool(rs.randint(0, 4) == 0)
        self.seed, self.base = int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 10 ** 6))
        self.small_block = bool(rs.randint(0, 2))
        self.fused = bool(rs.randint(0, 2))
        self.beams = int(rs.choice([4, 8]))
        self.fmt = [np.int16, np.int32, 'packed'][int(rs.randint(0, 3))]
        self.masks_on = bool(rs.randint(0, 2))
        self.caps = [int(rs.choice([n, 2 * n + 3])), max(n, 3 * self.A)]
        self.dev_forms = True
        self.settings = 'n=%d H=%d auto=%d prefetch=%s depth=%d term=%d base=%d block=%d lidar=%s/%d/%s masks=%d caps=%s' % (
            n, self.horizon, self.autoreset, self.prefetch, self.depth, self.term, self.base, self.small_block, 'fused' if self.fused else 'call', self.beams,
            getattr(self.fmt, '__name__', self.fmt), self.masks_on, self.caps)
        self.tag = '%s case %d (%s)' % (cfg, case, self.settings)
        from gym_novel_gridworlds_amd.lidar import LidarConfig
        self.lc = LidarConfig(spec, self.beams)
        self.cc = self.lc.compile(spec)
        zc = os.environ.pop('NGW_ZC_BYTES', None)        # the small page-locked block: set only around construction, then restored
        if self.small_block:
            os.environ['NGW_ZC_BYTES'] = '2048'
        try:
            self.v = make_env(spec=spec, num_envs=n, seed=self.seed, autoreset=self.autoreset, horizon=self.horizon, reset_prefetch=self.prefetch,
                              env_index_base=self.base, reset_prefetch_depth=self.depth, terminal_capture=self.term)
        finally:
            os.environ.pop('NGW_ZC_BYTES', None)
            if zc is not None:
                os.environ['NGW_ZC_BYTES'] = zc
        cs = spec.compile()
        self.o = NO.Oracle(cs, n, seed=self.seed, autoreset=self.autoreset, horizon=self.horizon, env_index_base=self.base)
        self.o2 = NO.Oracle(cs, n, autoreset=False)      # stepped beside the model where terminal rows are kept: the state an episode ended in
        self.snaps = [SO.NumpySnapshot(S, self.K, c) for c in self.caps]
        self.filled = [np.zeros(c, bool) for c in self.caps]      # never-saved slots are not read: a zero map has no walls to stop an agent
        self.table, self.book = KT.KeyTableModel(), KT.WhereBook(0)
        self.last_fields = 0                                 # the selection of the last call that inserted state keys into the table
        self.term_rows = dict(map=np.zeros((n, S * S), np.int8), loc=np.zeros((n, 2), np.int32), facing=np.zeros(n, np.int32), inv=np.zeros((n, self.K), np.int32))
        self.term_known = np.zeros(n, bool)
        self.ofail = 0
        self.flags = 0
        self.lidar_stale = False
        self.t_roll = 0
        self.graph = None

    # -------------------------------------------------------------- the model's own steps
    def mstep(self, a):
        """One batched step of the model; with terminal capture on, the rows the ended episodes ended in are kept."""
        o = self.o
        a = np.ascontiguousarray(a, np.int32)
        if self.term and self.autoreset:
            for dst, src in zip(self.o2.st.arrays() + [self.o2.st.episode], o.st.arrays() + [o.st.episode]):
                dst[...] = src
            self.o2.step(a)
        self.ofail |= int(o.step(a) != 0)
        if self.term and self.autoreset:
            idx = np.nonzero(o.done)[0]
            for k in ('map', 'loc', 'facing', 'inv'):
                self.term_rows[k][idx] = getattr(self.o2.st, k)[idx]
            self.term_known[idx] = True
        self.lidar_stale = False

    def dev(self, a):
        return self.v.to_device(np.ascontiguousarray(a))

    def maybe_dev(self, a, on):
        return self.dev(a) if on and a is not None else a

    def idx(self, a):
        return None if a is None else np.ascontiguousarray(a, np.int32)

    def both_reset(self, mask):
        v, o = self.v, self.o
        try:
            v.reset(mask)
        except AssertionError as ex:
            assert 'Cannot place items' in str(ex), self.tag
            assert (o.reset(mask) if mask is not None else o.reset()) != 0, self.tag + ': only the env under test failed to place'
            return False
        assert (o.reset(mask) if mask is not None else o.reset()) == 0, self.tag + ': only the oracle failed to place'
        self.lidar_stale = False
        return True

    # -------------------------------------------------------------- comparisons after every call
    def check_all(self, where, after_steps_injection=False):
        v, o = self.v, self.o
        hs = v.get_state()
        for k in STATE_KEYS:
            bad = np.nonzero((hs[k] != getattr(o.st, k)).reshape(self.n, -1).any(1))[0]
            assert bad.size == 0, "%s: %s differs for %d envs, first env %d" % (where, k, bad.size, bad[0])
        for i, (snap, model) in enumerate(zip(self.vsnaps, self.snaps)):
            XO.assert_rows(snap.state(), model.rows, '%s: snapshot %d' % (where, i))
        if self.fused and not self.lidar_stale:
            got = host(v.lidar_observation())
            got = v.lidar_widen(got) if isinstance(got, tuple) else got
            exp = NO.lidar(self.cc, self.S, self.K, o.st.map, o.st.loc, o.st.facing, o.st.inv)
            bad = np.nonzero((got != exp).any(1))[0]
            assert bad.size == 0, "%s: fused lidar rows differ for %d envs, first env %d" % (where, bad.size, bad[0])
        if self.masks_on:
            eq('action mask words', v.action_mask_words(), M.oracle_mask_words(self.spec, o.st), where)
        if after_steps_injection:
            return
        if self.term:
            got = v.terminal_observation()
            idx = np.nonzero(self.term_known)[0]
            for k, name in (('map', 'map'), ('loc', 'agent_location'), ('facing', 'agent_facing_id'), ('inv', 'inventory_items_quantity')):
                g = np.asarray(got[name]).reshape(self.n, -1)[idx]
                assert (g == self.term_rows[k].reshape(self.n, -1)[idx]).all(), "%s: terminal observation rows (%s) differ" % (where, name)
        assert v.error_flags() == self.flags, "%s: error flags %#x, the model says %#x" % (where, v.error_flags(), self.flags)

    # -------------------------------------------------------------- draws shared by the slot calls
    def draw_source(self, rs, max_pairs, dst=None, need_dst=True):
        """-> (source snapshot index or None for the live envs, destination snapshot index, parents, children): parents may repeat and name filled
        slots (or envs) only, children are distinct slots of the destination and, inside one buffer, disjoint from the parents."""
        from_envs = bool(rs.randint(0, 2))
        d = int(rs.randint(0, 2)) if dst is None else dst
        s = int(rs.randint(0, 2))
        c = int(rs.randint(1, max_pairs + 1))
        u, w = rs.randint(0, 1 << 30, c), rs.permutation(self.caps[d])
        if not self.filled[s].any():
            s = 0                                        # (snapshot 0 holds every env's state from the start of the case)
        if from_envs:
            parents, s = u % self.n, None
            children = w[:c]
        else:
            live = np.nonzero(self.filled[s])[0]
            parents = live[u % len(live)]
            free = w[~np.isin(w, parents)] if s == d else w
            if not len(free):                            # one buffer and no slot left beside the parents: the other snapshot takes the children
                d = 1 - d
                free = rs.permutation(self.caps[d])
            children = free[:c]
        if need_dst:
            parents = parents[:len(children)]
        return s, d, parents.astype(np.int32), children.astype(np.int32)

    def src_rows(self, s):
        return self.o.st if s is None else self.snaps[s]

    def src_kw(self, s, d):
        return dict(from_envs=True) if s is None else (dict(source=self.vsnaps[s]) if s != d else {})

    def write_children(self, d, children, ends):
        for k in STATE_KEYS:
            self.snaps[d].rows[k][children] = ends[k]
        self.filled[d][children] = True

    def filled_slots(self, rs, max_count):
        s = int(rs.randint(0, 2))
        u = rs.randint(0, 1 << 30, int(rs.randint(1, max_count + 1)))
        if not self.filled[s].any():
            s = 0
        live = np.nonzero(self.filled[s])[0]
        return s, live[u % len(live)].astype(np.int32)

    def envs_list(self, rs, max_count):
        """None (every env) one time in three, else a list with repeats."""
        u = rs.randint(0, 1 << 30, int(rs.randint(1, max_count + 1)))
        return None if rs.randint(0, 3) == 0 else (u % self.n).astype(np.int32)

    def draw_keys(self, rs, count):
        """Keys for the table's own calls: some it holds, some new, a zero, and repeats."""
        held = list(self.table.order)
        fresh = [int(x) for x in rs.randint(1, 1 << 62, count)]
        pick = rs.randint(0, 4, count)
        at = rs.randint(0, 1 << 30, count)
        keys = []
        for j in range(count):
            if pick[j] == 0 and held:
                keys.append(held[at[j] % len(held)])
            elif pick[j] == 1 and keys:
                keys.append(keys[at[j] % len(keys)])
            elif pick[j] == 2 and at[j] % 4 == 0:
                keys.append(0)
            else:
                keys.append(fresh[j])
        return np.array(keys, np.uint64)

    def draw_pad(self, rs, count, on_dev, kind):
        """The padding of one call's device index lists -> the bool [count] of the entries that become IDX_NONE, or None (a host list, an empty one, or
        two calls in three).  The side is kept in self.side for padded(); every draw is made whatever the outcome."""
        u, one = rs.rand(count), int(rs.randint(0, max(count, 1)))
        pad, layout, side = rs.randint(0, PAD_ONE_IN) == 0, PAD_LAYOUTS[int(rs.randint(0, len(PAD_LAYOUTS)))], PAD_SIDES[int(rs.randint(0, len(PAD_SIDES)))]
        if not (on_dev and pad and count):
            return None
        at = np.arange(count)
        if layout == 'wave' and count > 128:
            skip = (at >= 64) & (at < 128)
        elif layout in ('third', 'wave'):
            layout, skip = 'third', u < 1.0 / 3
        elif layout == 'but_one':
            skip = at != one
        else:
            skip = np.ones(count, bool)
        self.side = side
        self.log('(pad)', kind, (layout, side))
        return skip

    def pad_envs(self, rs, envs, on_dev, kind):
        """draw_pad for an env list -> (the list, the entries that become IDX_NONE or None); "None: every env" written out where it is padded."""
        skip = self.draw_pad(rs, self.n if envs is None else len(envs), on_dev, kind)
        return (np.arange(self.n, dtype=np.int32) if envs is None and skip is not None else envs), skip

    def padded(self, skip, src, dst=None):
        """The lists of a padded call: IDX_NONE in the source list, the destination list or both at the entries in `skip` (one list: that one)."""
        if skip is None:
            return (src, dst) if dst is not None else src
        if dst is None:
            return np.where(skip, NONE, src).astype(np.int32)
        return (np.where(skip & (self.side != 'destination'), NONE, src).astype(np.int32),
                np.where(skip & (self.side != 'source'), NONE, dst).astype(np.int32))

    def check_insert(self, keys, found, where):
        self.check_found(keys, self.table.insert(keys), found, where)

    def check_found(self, keys, model, found, where):
        fresh, stored = model
        assert len(self.table) <= TABLE_CAPACITY, "%s: the model holds %d keys, the table's capacity is %d" % (where, len(self.table), TABLE_CAPACITY)
        self.log('(table)', 'size', len(self.table))
        eq('fresh', host(found.fresh).reshape(-1), fresh, where)
        self.book.check(keys, host(found.where).reshape(-1), stored, where)
        assert len(self.vtable) == len(self.table), "%s: the table holds %d keys, the model %d" % (where, len(self.vtable), len(self.table))

    # -------------------------------------------------------------- the calls
    def call(self, kind, where):
        """Draws, predicts, performs and compares one call.  -> the form it took (for the coverage count) or raises Refused."""
        rs, v, o, n, A, spec = self.rs, self.v, self.o, self.n, self.A, self.spec
        on_dev = bool(rs.randint(0, 2))
        ar, H = self.autoreset, self.horizon
        form = ''
        if kind == 'step':
            for _ in range(int(rs.randint(1, 5))):
                a = rs.randint(0, A, size=n).astype(np.int32)
                self.mstep(a)
                obs, reward, done, info = v.step(a)
                assert (reward == o.reward).all() and (done == o.done.astype(bool)).all() and (info['message_code'] == o.msg_code).all(), where
                if not self.ofail:
                    assert (np.asarray(obs['map']).reshape(n, -1) == o.st.map).all() and (obs['inventory_items_quantity'] == o.st.inv).all(), where + ': host observation'
                    assert (obs['agent_location'] == o.st.loc).all() and (obs['agent_facing_id'] == o.st.facing).all(), where + ': host observation'
                    if self.fused:                        # the rows the host step itself delivered (write-through / copy behind the launch)
                        got = host(v.lidar_observation())
                        got = v.lidar_widen(got) if isinstance(got, tuple) else got
                        assert (got == NO.lidar(self.cc, self.S, self.K, o.st.map, o.st.loc, o.st.facing, o.st.inv)).all(), where + ': lidar rows of the host step'
        elif kind in ('dev', 'rollact'):
            k = int(rs.randint(1, MAX_STEPS + 1))
            an = rs.randint(0, A, size=(k, n)).astype(np.int32)
            acts = self.dev(an)
            for i in range(k):
                self.mstep(an[i])
            (v.step_device_many if kind == 'dev' else v.rollout_actions)(v.ptr_of(acts), n, k)
        elif kind == 'rollout':
            k = int(rs.randint(1, 30))
            if not ar and rs.randint(0, 2):
                k = 1 + k % 4
            before = o.st.episode.copy()
            self.ofail |= int(o.rollout(k, self.seed ^ 77, self.t_roll) != 0)
            v.rollout(k, action_seed=self.seed ^ 77, t0=self.t_roll)
            self.t_roll += k
            self.term_known &= o.st.episode == before     # (generated actions: the model has no per-step view of where these episodes ended)
            self.lidar_stale = False
        elif kind in ('reset', 'mask_reset'):
            m = (rs.randint(0, 3, size=n) == 0).astype(np.uint8) if kind == 'mask_reset' else None
            if not self.both_reset(m):
                return None
        elif kind == 'state_steps':
            sc = rs.randint(0, max(H, 5), size=n).astype(np.int32)
            v.set_state(0, step_count=sc)
            o.st.step_count[:] = sc
        elif kind == 'state_rows':                          # map, pose and inventory rows of other envs of the model, over a run of envs
            m = int(rs.randint(1, n + 1))
            first = int(rs.randint(0, n - m + 1))
            src = rs.randint(0, n, m)
            rows = {k: getattr(o.st, k)[src].copy() for k in ('map', 'loc', 'inv')}
            v.set_state(first, map=rows['map'], loc=rows['loc'], inv=rows['inv'])
            for k in rows:
                getattr(o.st, k)[first:first + m] = rows[k]
            self.lidar_stale = True                       # (no launch: the fused rows are the last launch's)
        elif kind == 'step_sampled':
            w = SA.random_weights(rs, n, A)
            seed, t = int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 1000))
            exp = SA.oracle_sample(spec, o.st, np.arange(n), w, seed, self.base, t)
            self.mstep(exp[0])
            got = v.step_sampled(self.dev(np.ascontiguousarray(w.T)) if on_dev else w, seed, t)
            v.sync()
            g = host(tuple(got))
            SA.assert_sampled((g[0], g[1], same_bits(g[2], np.zeros(0, np.uint64))), exp, where)
        elif kind == 'restore':
            keep = bool(rs.randint(0, 2))
            s, slots = self.filled_slots(rs, n)
            envs = rs.permutation(n)[:len(slots)].astype(np.int32)
            if self.filled[s][:n].all() and self.caps[s] >= n and rs.randint(0, 4) == 0:
                slots = envs = None                       # the whole batch, no lists
            else:
                slots = slots[:len(envs)]
            skip = None if slots is None else self.draw_pad(rs, len(slots), on_dev, kind)
            if skip is None:
                self.snaps[s].restore(o.st, slots, envs, keep)
            else:                                          # "makes that one copy a no-op": the live copies alone
                self.snaps[s].restore(o.st, slots[~skip], envs[~skip], keep)
                slots, envs = self.padded(skip, slots, envs)
            self.vsnaps[s].restore(slots=self.maybe_dev(slots, on_dev), envs=self.maybe_dev(envs, on_dev), keep_episode=keep)
            self.lidar_stale = False
            form = 'keep' if keep else 'episode'
        elif kind == 'fork':
            keep = bool(rs.randint(0, 2))
            src = rs.randint(0, n, n).astype(np.int32)
            skip = self.draw_pad(rs, n, on_dev, kind)
            tmp = SO.NumpySnapshot(self.S, self.K, n)
            tmp.save(o.st)
            if skip is None:
                tmp.restore(o.st, src, None, keep)
            else:                                          # an env whose source is not there stays as it is
                tmp.restore(o.st, src[~skip], np.arange(n)[~skip], keep)
            v.fork(self.maybe_dev(self.padded(skip, src), on_dev), keep_episode=keep)
            self.lidar_stale = False
        elif kind == 'graph_launch':
            reps = int(rs.randint(1, 3))
            for _ in range(reps):
                for a in self.graph[0]:
                    self.mstep(a)
            v.graph_launch(reps)
        elif kind == 'save':
            d = int(rs.randint(0, 2))
            c = int(rs.randint(1, min(n, self.caps[d]) + 1))
            envs, slots = rs.randint(0, n, c).astype(np.int32), rs.permutation(self.caps[d])[:c].astype(np.int32)
            skip = self.draw_pad(rs, c, on_dev, kind)
            live = slice(None) if skip is None else ~skip
            self.snaps[d].save(o.st, envs[live], slots[live])
            self.filled[d][slots[live]] = True
            envs, slots = self.padded(skip, envs, slots)
            self.vsnaps[d].save(envs=self.maybe_dev(envs, on_dev), slots=self.maybe_dev(slots, on_dev))
        elif kind == 'copy':
            s, d, src, dst = self.draw_source_slots(rs)
            skip = self.draw_pad(rs, len(src), on_dev, kind)
            live = slice(None) if skip is None else ~skip
            for k in STATE_KEYS:
                self.snaps[d].rows[k][dst[live]] = self.snaps[s].rows[k][src[live]]
            self.filled[d][dst[live]] = True
            src, dst = self.padded(skip, src, dst)
            self.vsnaps[d].copy(self.maybe_dev(src, on_dev), self.maybe_dev(dst, on_dev), source=None if s == d else self.vsnaps[s])
            form = 'within' if s == d else 'between'
        elif kind == 'expand':
            s, d, parents, children = self.draw_source(rs, MAX_PAIRS)
            actions = rs.randint(0, A, len(parents)).astype(np.int32)
            skip = self.draw_pad(rs, len(parents), on_dev, kind)
            live = slice(None) if skip is None else ~skip
            kids, rep = XO.oracle_expand(spec, rows_of(self.src_rows(s)), parents, actions, ar, H)
            self.write_children(d, children[live], {k: kids[k][live] for k in STATE_KEYS})
            if skip is not None:                           # "nothing is stored, its reports are left untouched": the zeros they were allocated as
                rep = {k: np.where(skip, np.zeros((), x.dtype), x) for k, x in rep.items()}
            p, c = self.padded(skip, parents, children)
            got = self.vsnaps[d].expand(self.maybe_dev(p, on_dev), self.maybe_dev(actions, on_dev), self.maybe_dev(c, on_dev), device=on_dev,
                                        **self.src_kw(s, d))
            for k in ('reward', 'done', 'result', 'info'):
                eq(k, got[k], rep[k], where)
            form = 'envs' if s is None else 'slots'
        elif kind == 'expand_all':
            s, _, parents, _ = self.draw_source(rs, 3, dst=1, need_dst=False)
            if s == 1:                                    # (the children go to snapshot 1: the parents come from the envs or snapshot 0)
                s, parents = 0, (parents % n).astype(np.int32)
            first = int(rs.randint(0, self.caps[1] - len(parents) * A + 1))
            pp, aa = np.repeat(parents, A), np.tile(np.arange(A), len(parents))
            kids, rep = XO.oracle_expand(spec, rows_of(self.src_rows(s)), pp, aa, ar, H)
            self.write_children(1, first + np.arange(len(pp)), kids)
            got = self.vsnaps[1].expand_all(self.maybe_dev(parents, on_dev), first, device=on_dev, **self.src_kw(s, 1))
            for k in ('reward', 'done', 'result', 'info'):
                eq(k, host(got[k]).reshape(-1), rep[k], where)
                assert tuple(got[k].shape) == (len(parents), A), where
            form = 'envs' if s is None else 'slots'
        elif kind in ('srollout', 'srollout_kids', 'splayout', 'splayout_kids'):
            form = self.pair_call(kind, where, on_dev)
        elif kind in GUIDED_KINDS:
            form = self.guided_call(kind, where, on_dev)
        elif kind == 'playouts':
            form = PLAYOUTS_FORMS[int(rs.randint(0, len(PLAYOUTS_FORMS)))]
            P = int(rs.randint(1, min(MAX_PLANS, MAX_PAIRS // n) + 1))
            if form == 'guided':
                return self.guided_call(kind, where, on_dev, P)
            steps, seed = int(rs.randint(1, MAX_STEPS + 1)), int(rs.randint(0, 2 ** 31))
            w = (rs.rand(A) * (rs.rand(A) < 0.8)).astype(np.float32)
            fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
            V = int(rs.choice(VIEW_SIZES))
            kw, rkw = {}, {}
            if form == 'view':                              # a 'rewards' call with the AgentMap views of every visited row
                kw.update(rewards=True, observe='agent_view', view_size=V); rkw.update(rewards=True, view_size=V)
            elif form == 'weights':
                kw['weights'], rkw['weights'] = (self.dev(w) if on_dev else w), w
            elif form == 'path_keys':
                kw.update(path_keys=True, fields=fields); rkw.update(path_keys=True, fields=fields)
            elif form == 'rewards':
                kw['rewards'] = rkw['rewards'] = True
            elif form == 'masks':
                kw['masks'] = rkw['masks'] = True
            elif form == 'observe':
                kw['observe'], rkw['lc'] = 'lidar', self.lc
            exp = ref_pairs(spec, rows_of(o.st), np.repeat(np.arange(n), P), 'playout', ar, H, steps=steps, seed=seed, first_pair=self.base * P, **rkw)
            got = v.playouts(P, steps, seed, device=on_dev, **kw)
            assert tuple(got.ret.shape) == (n, P), where
            check_pairs(got, exp, 'playout', False, where)
        elif kind == 'mask_words':
            eq('action mask words', v.action_mask_words(device=on_dev, copy=bool(rs.randint(0, 2))), M.oracle_mask_words(spec, o.st), where)
        elif kind == 'lookahead':
            exp = LO.oracle_lookahead(spec, o.st, ar, H)
            got = v.lookahead(device=on_dev, copy=bool(rs.randint(0, 2)))
            for k in ('reward', 'done', 'result', 'info'):
                eq(k, got[k], exp[k], where)
        elif kind == 'plans':
            P, steps = int(rs.randint(1, MAX_PLANS + 1)), int(rs.randint(1, MAX_STEPS + 1))
            plans = rs.randint(0, A, (n, P, steps)).astype(np.int32)
            exp = PL.oracle_plans(spec, o.st, plans, ar, H)
            got = v.evaluate_plans(self.dev(np.ascontiguousarray(plans.transpose(2, 1, 0))) if on_dev else plans, device=bool(rs.randint(0, 2)))
            for k in ('ret', 'length', 'ended', 'info'):
                eq(k, got[k], exp[k], where)
        elif kind in ('state_keys', 'insert_state_keys'):
            envs = self.envs_list(rs, MAX_PAIRS)
            fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
            exp = fast_keys(rows_at(o.st, np.arange(n) if envs is None else envs), fields)
            envs, skip = self.pad_envs(rs, envs, on_dev, kind)
            if skip is not None:                           # "that key is 0"
                exp, envs = np.where(skip, np.uint64(0), exp), self.padded(skip, envs)
            if kind == 'state_keys':
                eq('keys', v.state_keys(self.maybe_dev(envs, on_dev), fields, device=on_dev), exp, where)
            else:
                keys, found = v.insert_state_keys(self.vtable, self.maybe_dev(envs, on_dev), fields, device=on_dev)
                eq('keys', keys, exp, where)
                self.check_insert(exp, found, where)
                self.last_fields = fields
        elif kind in ('succ_keys', 'insert_succ_keys'):
            envs = self.envs_list(rs, MAX_PAIRS if kind == 'succ_keys' else 8)
            if kind == 'insert_succ_keys' and envs is None:
                envs = np.arange(min(n, 8), dtype=np.int32)
            fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
            reports = bool(rs.randint(0, 4))
            envs, skip = self.pad_envs(rs, envs, on_dev, kind)
            if self.S > SUCC_MAX_MAP:
                from gym_novel_gridworlds_amd.snapshot import MapsTooLarge
                raise Refused(MapsTooLarge)
            ex = SU.Successors(spec, o.st, np.arange(n) if envs is None else envs, ar, H)
            zero = () if skip is None else np.nonzero(skip)[0]        # a parent that is not there: its A keys are 0, its reports are 0
            envs = envs if skip is None else self.padded(skip, envs)
            if kind == 'succ_keys':
                SU.assert_successors(v.successor_keys(self.maybe_dev(envs, on_dev), fields, device=on_dev, reports=reports), ex, fields, where, reports, zero)
            else:
                got, found = v.insert_successor_keys(self.vtable, self.maybe_dev(envs, on_dev), fields, device=on_dev)
                SU.assert_successors(got, ex, fields, where, True, zero)
                assert tuple(found.fresh.shape) == tuple(ex.keys(fields).shape), where
                keys = ex.keys(fields).copy()
                keys[list(zero)] = 0
                self.check_insert(keys.reshape(-1), found, where)
                self.last_fields = fields
        elif kind == 'table_insert':
            keys = self.draw_keys(rs, int(rs.randint(1, 65)))
            found = self.vtable.insert(self.dev(keys.view(np.int64)) if on_dev else (keys if rs.randint(0, 2) else keys.view(np.int64)), device=on_dev)
            self.check_insert(keys, found, where)
        elif kind == 'table_lookup':
            keys = self.draw_keys(rs, int(rs.randint(1, 65)))
            where_ = self.vtable.lookup(self.dev(keys.view(np.int64)) if on_dev else keys, device=on_dev)
            self.book.check(keys, host(where_), self.table.contains(keys), where)
            assert len(self.vtable) == len(self.table), where
        elif kind == 'sample':
            envs = self.envs_list(rs, MAX_PAIRS)
            idx = np.arange(n) if envs is None else envs
            w = SA.random_weights(rs, len(idx), A)
            seed, t = int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 1000))
            envs, skip = self.pad_envs(rs, envs, on_dev, kind)
            exp = SA.oracle_sample(spec, o.st, idx, w, seed, self.base, t)
            if skip is not None:                           # "that pair gets action -1, mass 0 and mask 0"
                exp = (np.where(skip, -1, exp[0]).astype(np.int32), np.where(skip, np.float32(0), exp[1]), np.where(skip, np.uint64(0), exp[2])) + exp[3:]
                envs = self.padded(skip, envs)
            got = v.sample_actions(self.dev(np.ascontiguousarray(w.T)) if on_dev else w, seed, t, self.maybe_dev(envs, on_dev), device=on_dev)
            g = host(tuple(got))
            SA.assert_sampled((g[0], g[1], same_bits(g[2], np.zeros(0, np.uint64))), exp, where)
        elif kind in ('slot_lidar', 'slot_view', 'slot_masks', 'slot_keys', 'slot_unique', 'slot_insert_keys'):
            s, slots = self.filled_slots(rs, MAX_PAIRS)
            snap, rows = self.vsnaps[s], self.snaps[s].rows
            fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
            V = int(rs.choice([1, 2, 5]))
            skip = None if kind == 'slot_unique' else self.draw_pad(rs, len(slots), on_dev, kind)
            arg = self.maybe_dev(self.padded(skip, slots), on_dev)
            if skip is not None and kind in ('slot_lidar', 'slot_view', 'slot_masks'):
                # "its output row is all zeros (mask 0, facing 0)": the references' rows with zeros in the places of the slots that are not there
                if kind == 'slot_lidar':
                    got = host(snap.lidar_observation(arg, device=on_dev))
                    got, exp = {'lidar': v.lidar_widen(got) if isinstance(got, tuple) else got}, {'lidar': OO.expect_lidar(spec, self.lc, rows, slots)}
                elif kind == 'slot_view':
                    got, exp = OO.host(snap.agent_view(arg, V, device=on_dev)), OO.expect_view(rows, slots, V)
                else:
                    got, exp = {'masks': host(snap.action_masks(arg, device=on_dev))}, {'masks': OO.expect_masks(spec, rows, slots)}
                    assert got['masks'].dtype == np.bool_, where
                assert sorted(got) == sorted(exp), where
                for k in exp:
                    e = np.array(exp[k])
                    e[skip] = 0
                    assert kind == 'slot_lidar' or got[k].dtype == e.dtype, (where, k, got[k].dtype)
                    eq(k, got[k], e, where)
            elif kind == 'slot_lidar':
                OO.assert_lidar(v, snap.lidar_observation(arg, device=on_dev), spec, self.lc, rows, slots, where)
            elif kind == 'slot_view':
                OO.assert_view(snap.agent_view(arg, V, device=on_dev), rows, slots, V, where)
            elif kind == 'slot_masks':
                OO.assert_masks(snap.action_masks(arg, device=on_dev), spec, rows, slots, where)
            else:
                exp = fast_keys(rows_at(self.snaps[s], slots), fields)
                if skip is not None:
                    exp = np.where(skip, np.uint64(0), exp)
                if kind == 'slot_keys':
                    eq('keys', snap.keys(arg, fields, device=on_dev), exp, where)
                elif kind == 'slot_unique':
                    first, inverse = host(tuple(snap.unique(arg, fields, device=on_dev)))
                    seen = {}
                    want = np.array([seen.setdefault(int(k), j) for j, k in enumerate(exp.tolist())], np.int64)
                    eq('unique: the first position of every group', np.asarray(first)[np.asarray(inverse)], want, where)
                    assert len(first) == len(seen), where
                else:
                    keys, found = snap.insert_keys(self.vtable, arg, fields, device=on_dev)
                    eq('keys', keys, exp, where)
                    self.check_insert(exp, found, where)
                    self.last_fields = fields
        elif kind == 'agent_view':
            V = int(rs.choice([1, 2, 5]))
            eq('agent view', v.agent_view(V, device=on_dev, copy=bool(rs.randint(0, 2))), NO.agent_view(o.st.map, o.st.loc, V), where)
        elif kind == 'lidar':
            got = host(v.lidar_observation(device=on_dev))
            if not (self.fused and self.lidar_stale):     # (fused: the rows are the last launch's, and set_state launches nothing)
                eq('lidar rows', v.lidar_widen(got) if isinstance(got, tuple) else got, NO.lidar(self.cc, self.S, self.K, o.st.map, o.st.loc, o.st.facing, o.st.inv), where)
        elif kind in ('slot_walk', 'walk'):
            form = self.walk_call(kind, where, on_dev)
        elif kind == 'walk_go':
            form = self.walk_go(kind, where)
        elif kind == 'frontier_compact':
            form = self.frontier_compact(kind, where)
        elif kind == 'frontier_step':
            form = self.frontier_step(kind, where)
        elif kind == 'frontier_twins':
            form = self.guided_call(kind, where, True, twins=True)
        else:
            raise AssertionError('unknown call kind ' + kind)
        return form

    def draw_source_slots(self, rs):
        """A slot-to-slot copy: -> (source snapshot, destination snapshot, src slots - filled, may repeat -, dst slots - distinct, and inside one
        buffer no source)."""
        s, d = int(rs.randint(0, 2)), int(rs.randint(0, 2))
        c = int(rs.randint(1, min(MAX_PAIRS, max(1, self.caps[d] // 2)) + 1))
        u, w = rs.randint(0, 1 << 30, c), rs.permutation(self.caps[d])
        if not self.filled[s].any():
            s = 0
        live = np.nonzero(self.filled[s])[0]
        src = live[u % len(live)]
        free = w[~np.isin(w, src)] if s == d else w
        if not len(free):
            d = 1 - d
            free = rs.permutation(self.caps[d])
        dst = free[:c]
        return s, d, src[:len(dst)].astype(np.int32), dst.astype(np.int32)

    def pair_call(self, kind, where, on_dev):
        """Snapshot.rollout / Snapshot.playout, with and without children, every form from slots and from the live envs."""
        rs, spec, A = self.rs, self.spec, self.A
        playout, kids = kind.startswith('splayout'), kind.endswith('_kids')
        forms = PLAYOUT_FORMS if playout else ROLLOUT_FORMS
        form = forms[int(rs.randint(0, len(forms)))]
        s, d, parents, children = self.draw_source(rs, MAX_PAIRS, need_dst=kids)
        if not kids:
            children = None
        count = len(parents)
        steps, seed, first_pair = int(rs.randint(1, MAX_STEPS + 1)), int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 40))
        plans = rs.randint(0, A, (count, steps)).astype(np.int32)
        w = (rs.rand(A) * (rs.rand(A) < 0.8)).astype(np.float32)
        limits = rs.randint(0, steps + 1, count).astype(np.int32) if rs.randint(0, 2) else None
        fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
        record, with_keys, with_obs, with_masks = bool(rs.randint(0, 2)), bool(rs.randint(0, 2)), bool(rs.randint(0, 2)), bool(rs.randint(0, 2))
        V = int(rs.choice(VIEW_SIZES))
        kw, rkw = {}, {}
        if form == 'weighted' or (playout and form != 'plain' and rs.randint(0, 3) == 0):
            kw['weights'], rkw['weights'] = (self.dev(w) if on_dev else w), w
        if form in ('path', 'traj', 'view'):
            if limits is not None:
                kw['limits'], rkw['limits'] = self.maybe_dev(limits, on_dev), limits
            if with_keys or (form == 'path' and limits is None):
                kw.update(path_keys=True, fields=fields); rkw.update(path_keys=True, fields=fields)
        if form in ('traj', 'view'):                        # 'view': a 'traj' call whose observation is the AgentMap dict, always asked for
            kw['rewards'] = rkw['rewards'] = True
            if form == 'view':
                kw.update(observe='agent_view', view_size=V); rkw['view_size'] = V
            elif with_obs:
                kw['observe'], rkw['lc'] = 'lidar', self.lc
            if playout and with_masks:
                kw['masks'] = rkw['masks'] = True
        skip = self.draw_pad(rs, count, on_dev, kind)
        live = slice(None) if skip is None else ~skip
        # (the pairs of one call do not see each other, and a playout's draws go by the pair's position: the references run on the list as drawn,
        # and the pairs that are not there get what the contract stores for them)
        if playout:
            exp = ref_pairs(spec, rows_of(self.src_rows(s)), parents, 'playout', self.autoreset, self.horizon, steps=steps, seed=seed, first_pair=first_pair, **rkw)
        else:
            exp = ref_pairs(spec, rows_of(self.src_rows(s)), parents, 'rollout', self.autoreset, self.horizon, plans=plans, **rkw)
        if kids:
            self.write_children(d, children[live], {k: exp['ends'][k][live] for k in STATE_KEYS})
        exp = blank_pairs(exp, skip)
        snap, src = self.vsnaps[d], self.src_kw(s, d)
        if skip is not None:
            parents, children = self.padded(skip, parents, children) if kids else (self.padded(skip, parents), None)
        p, c = self.maybe_dev(parents, on_dev), self.maybe_dev(children, on_dev)
        if playout:
            got = snap.playout(p, steps, seed, children=c, first_pair=first_pair, record=record, device=on_dev, **src, **kw)
        else:
            got = snap.rollout(p, self.dev(np.ascontiguousarray(plans.T)) if on_dev else plans, children=c, device=on_dev, **src, **kw)
        check_pairs(got, exp, 'playout' if playout else 'rollout', record, where)
        return '%s/%s' % (form, 'envs' if s is None else 'slots')

    def guided_call(self, kind, where, on_dev, P=None, twins=False):
        """A guided playout - Snapshot.playout(table=, table_weights=, outside=) with or without children, or with P the 'guided' form of playouts()
        - over the case's own table: whatever the earlier calls inserted, under whatever fields, plus (three times in four) an offer of keys under this
        call's fields.  Every row of table_weights no member owns is NaN: a lane that reads one changes the actions or raises F_BAD_WEIGHT."""
        rs, spec, A, n, ar, H = self.rs, self.spec, self.A, self.n, self.autoreset, self.horizon
        batch, kids = P is not None, kind.endswith('_kids')
        # 1. every draw
        s, d, parents, children = self.draw_source(rs, MAX_PAIRS, need_dst=kids)
        steps, seed, first_pair = int(rs.randint(1, MAX_STEPS + 1)), int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 40))
        if batch:
            s, parents, first_pair = None, np.repeat(np.arange(n), P).astype(np.int32), self.base * P
        if not kids:
            children = None
        count = len(parents)
        fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
        limits = rs.randint(0, steps + 1, count).astype(np.int32) if rs.randint(0, 2) and not batch else None
        w = (rs.rand(A) * (rs.rand(A) < 0.8)).astype(np.float32)
        default = w if rs.randint(0, 3) else None
        outside = ('default', 'stop')[int(rs.randint(0, 2))]
        record, with_keys, rewards, masks = [bool(x) for x in rs.randint(0, 2, 4)]
        if twins:                                        # what the three twins read: the recorded actions, the path keys, a per-step field
            record = with_keys = rewards = True
        observe =(None, None, 'lidar', 'agent_view')[int(rs.randint(0, 4))]
        V = int(rs.choice(VIEW_SIZES))
        fill_seed = int(rs.randint(0, 2 ** 31))
        offer, again = bool(rs.randint(0, 4)), bool(rs.randint(0, 2))
        if not offer and again and self.last_fields:     # a table only earlier calls filled, looked up under the selection the last of them keyed it by
            fields = self.last_fields
        keep = rs.rand(count * (1 + (steps + 1) // 2)) < OFFER_KEEP[int(rs.randint(0, len(OFFER_KEEP)))]
        probe = rs.randint(0, 1 << 30, 64)
        skip = self.draw_pad(rs, count, on_dev and not batch, kind)
        record = record and not batch                    # (playouts() records no actions)
        src = self.src_rows(s)
        rows = rows_of(src)
        # 2. the offer: the parents' keys and the path keys of the even steps of a plain playout under the fill seed (guided_playout_oracle.inputs'
        #    recipe), thinned, through the table's own insert
        bound = False
        if offer:
            _, _, acts, _ = PO.oracle_playout(spec, rows, parents, steps, fill_seed, 0, ar, H)
            _, _, _, states, _ = KO.oracle_path(spec, rows, parents, acts, None, ar, H, fields)
            at = [(t, j) for t in range(0, steps, 2) for j in range(count) if (t, j) in states]
            path = fast_keys({k: np.stack([np.asarray(states[i][k]) for i in at]) for k in STATE_KEYS}, fields) if at else np.zeros(0, np.uint64)
            keys = np.concatenate([fast_keys(rows_at(src, parents), fields), path])
            keys = keys[keep[:len(keys)]]
            new = set(keys.tolist()) - set(self.table.order) - {0}
            bound = len(self.table) + len(new) > TABLE_CAPACITY
            if len(keys) and not bound:                  # (a full table is not what this fuzz models: both sides skip the offer)
                self.check_insert(keys, self.vtable.insert(keys), where + ' (the offer)')
                self.last_fields = fields
        # 3. the weight rows: f(key) in the bucket the table reported for that key (never a fresh look-up), NaN everywhere else
        craft = GO.craft_ids(spec)
        members = list(self.table.order)
        tw = np.full((self.vtable.buckets, A), np.nan, np.float32)
        for k in members:
            tw[self.book.of_key[k]] = GO.row_of(k, A, craft)
        # 4. the expectation
        e = GO.oracle_guided(spec, rows, parents, steps, seed, members, lambda k: GO.row_of(k, A, craft), default, first_pair, ar, H, fields, limits,
                             outside == 'stop', self.lc if observe == 'lidar' else None)
        assert not e['bad'], where + ': the model itself read a bad weight'
        exp = dict(ends=e['ends'], rep=dict(e['reports'], first_action=e['actions'][0].copy()), actions=e['actions'], keys=None,
                   rewards=e['rewards'] if rewards else None, masks=e['masks'] if masks else None, obs=e['obs'])
        if observe == 'agent_view':
            exp['obs'] = VO.expect_views(spec, rows, parents, e, V)
        if with_keys:                                    # hashed here from the visited rows, as ref_pairs does
            exp['keys'] = np.zeros((steps, count), np.uint64)
            at = sorted(e['states'])
            if at:
                kk = fast_keys({k: np.stack([np.asarray(e['states'][i][k]) for i in at]) for k in STATE_KEYS}, fields)
                for (t, j), x in zip(at, kk):
                    exp['keys'][t, j] = x
        ran = e['actions'] >= 0
        exp_where = np.full((steps, count), -1, np.int32)
        for t, j in np.argwhere(e['hit']):
            exp_where[t, j] = self.book.of_key[int(e['before'][t, j])]
        exp_depth = e['depth']
        live = slice(None) if skip is None else ~skip
        if kids:
            self.write_children(d, children[live], {k: e['ends'][k][live] for k in STATE_KEYS})
        if skip is not None:                             # the pairs that are not there: blank_pairs' values, where -1, "depth 0 for a skipped pair"
            exp = blank_pairs(exp, skip)
            exp_where, exp_depth = np.where(skip[None, :], -1, exp_where).astype(np.int32), np.where(skip, 0, exp_depth)
            parents, children = self.padded(skip, parents, children) if kids else (self.padded(skip, parents), None)
        # the call
        kw = dict(table=self.vtable, table_weights=self.dev(tw) if on_dev else tw, outside=outside, fields=fields, rewards=rewards, masks=masks)
        if default is not None:
            kw['weights'] = self.dev(default) if on_dev else default
        if with_keys:
            kw['path_keys'] = True
        if observe is not None:
            kw['observe'] = observe
        if observe == 'agent_view':
            kw['view_size'] = V
        if batch:
            got = self.v.playouts(P, steps, seed, device=on_dev, **kw)
            assert tuple(got.ret.shape) == (n, P) and tuple(got.where.shape) == (steps, n, P) and tuple(got.depth.shape) == (n, P), where
        else:
            if limits is not None:
                kw['limits'] = self.maybe_dev(limits, on_dev)
            got = self.vsnaps[d].playout(self.maybe_dev(parents, on_dev), steps, seed, children=self.maybe_dev(children, on_dev), first_pair=first_pair,
                                         record=record, device=on_dev, **self.src_kw(s, d), **kw)
        assert type(got).__name__ == 'PlayoutGuided', "%s: a %s came back" % (where, type(got).__name__)
        check_pairs(got, exp, 'playout', record, where)
        for name, x in (('where', exp_where), ('depth', exp_depth)):
            g = host(getattr(got, name))
            assert g.dtype == np.int32, "%s: %s is %s" % (where, name, g.dtype)
            eq(name, g.reshape(x.shape), x, where)
        # the call commits nothing to the table: its count, and the buckets of up to 64 members
        assert len(self.vtable) == len(self.table), "%s: the table holds %d keys, the model %d" % (where, len(self.vtable), len(self.table))
        if members:
            held = np.array([members[i % len(members)] for i in probe[:min(64, len(members))]], np.uint64)
            self.book.check(held, host(self.vtable.lookup(held)), np.ones(len(held), bool), where + ' (members after the call)')
        home = GO.home_buckets(np.array(members, np.uint64), self.vtable.buckets) if members else np.zeros(0, np.int64)
        ev = e['events']
        self.log('(guided)', kind, tuple(sorted(dict(
            outside=outside, source='envs' if s is None else 'slots', limits=limits is not None, observe=observe, default=default is not None,
            offered=offer, bound=bound, S=self.S, members=len(members), hits=ev['hits'], misses=ev['misses'], executed=ev['executed'],
            reentries=ev['reentries'], zero_mass=ev['zero_mass'], differs=ev['differs'], key0=int((ran & (e['before'] == 0)).sum()),
            displaced=int((home != np.array([self.book.of_key[k] for k in members], np.int64)).sum()),
            shared_home=len(members) - len(set(home.tolist()))).items())))
        if twins:
            self.twins(got, exp, exp_where, steps, count, where)
        return 'guided' if batch else 'guided/%s' % ('envs' if s is None else 'slots')

    def twins(self, got, exp, exp_where, steps, count, where):
        """'frontier_twins': the padded twins of the dense helpers on a device-form guided playout recorded with record=True - fr.fresh_steps (of the
        `fresh` flags the table reports for the call's path keys), fr.transitions(result), fr.tree_steps(result) - against the same lists computed from
        the model's expected result and padded by frontier_oracle, each at a capacity below, at and above the hits."""
        keys = exp['keys'].reshape(-1)
        new = set(keys.tolist()) - set(self.table.order) - {0}
        if len(self.table) + len(new) <= TABLE_CAPACITY:
            model = self.table.insert(keys)
            found = self.vtable.insert(got.keys.reshape(-1), device=True)
            self.check_found(keys, model, found, where + ' (the path keys)')
            e_fresh, fresh = model[0].reshape(steps, count), found.fresh.reshape(steps, count)
        else:                                            # (a full table is not what this fuzz models: the flags are the executed steps' keys)
            e_fresh, fresh = exp['keys'] != 0, got.keys.reshape(steps, count) != 0
        fresh = fresh.contiguous() if hasattr(fresh, 'contiguous') else fresh
        e_ran = np.arange(steps)[:, None] < exp['rep']['length'][None, :]
        e_tree = exp_where >= 0
        n = max(count, 1)
        pool = self.vsnaps[0]
        for name, flags in (('fresh_steps', e_fresh), ('transitions', e_ran), ('tree_steps', e_tree)):
            hits = int(np.count_nonzero(flags))
            for capacity in sorted({max(hits - 1, 0), hits, hits + 70}):
                w = '%s, %s at capacity %d of %d hits' % (where, name, capacity, hits)
                e_t, e_j, e_count, full = FO.compact(flags, n, None, capacity)
                fr = pool.frontier(capacity)
                if name == 'tree_steps':
                    bucket, action, t, j = fr.tree_steps(got)
                    live = e_t != NONE
                    eq('bucket', bucket, np.where(live, exp_where[e_t * live, e_j * live], NONE).astype(np.int32), w)
                    eq('action', action, np.where(live, exp['actions'][e_t * live, e_j * live], NONE).astype(np.int32), w)
                else:
                    t, j = fr.fresh_steps(fresh) if name == 'fresh_steps' else fr.transitions(got)
                eq('t', t, e_t, w)
                eq('j', j, e_j, w)
                eq('count', fr.count_dev, np.array(e_count, np.int32), w)
                self.raise_full(full, w)
                fr.close()
        self.log('(twins)', 'frontier_twins', (int(np.count_nonzero(e_fresh)), int(np.count_nonzero(e_ran)), int(np.count_nonzero(e_tree))))

    # -------------------------------------------------------------- walk distances and go-to plans
    def walk_rows_max(self):
        return MAX_PAIRS if self.S <= 16 else WALK_ROWS_LARGE

    def expect_walk(self, rows, idx, items, steps, skip):
        """walk_oracle's (dist, plans, length) of rows idx; "every output of that row is -1" for a row that is not there."""
        dist, plans, length = WO.walk_rows(rows, idx, self.K, items, steps, walk_ids(self.spec.compile()))
        if skip is not None:
            dist = np.where(skip[:, None], -1, dist).astype(np.int32)
            if items is not None:
                plans, length = np.where(skip[None, :], -1, plans).astype(np.int32), np.where(skip, -1, length).astype(np.int32)
        return dist, plans, length

    def walk_call(self, kind, where, on_dev):
        """Snapshot.walk_distances / walk_plans on filled slots ('slot_walk'), VecNovelGridworld's on the live envs ('walk'): host and device lists, every
        item id below K, plans complete and cut short."""
        rs, n, K = self.rs, self.n, self.K
        if kind == 'slot_walk':
            s, idx = self.filled_slots(rs, self.walk_rows_max())
            arg, rows, target = idx, self.snaps[s].rows, self.vsnaps[s]
        else:
            arg = self.envs_list(rs, self.walk_rows_max())
            if arg is None and n > self.walk_rows_max():  # (every env of a large map: too many rows for the oracle)
                arg = np.arange(self.walk_rows_max(), dtype=np.int32)
            idx, rows, target = (np.arange(n) if arg is None else arg), rows_of(self.o.st), self.v
        count = len(idx)
        plans_on = bool(rs.randint(0, 3)) and None not in walk_ids(self.spec.compile())
        steps, items = int(rs.randint(1, WALK_STEPS + 1)), rs.randint(0, K, count).astype(np.int32)
        one_item, item_list = bool(rs.randint(0, 4) == 0), bool(rs.randint(0, 2))
        if one_item:
            items[:] = items[0]
        arg, skip = self.pad_envs(rs, arg, on_dev, kind) if kind == 'walk' else (arg, self.draw_pad(rs, count, on_dev, kind))
        dist, plans, length = self.expect_walk(rows, idx, items if plans_on else None, steps, skip)
        it = int(items[0]) if one_item else self.maybe_dev(items, on_dev)
        if skip is not None:                             # the row, the item or both are not there (the distances alone, one item for all: the row)
            if plans_on and not one_item:
                arg, it = self.padded(skip, arg, items)
                it = self.dev(it)
            else:
                arg = self.padded(skip, arg)
        arg = self.maybe_dev(arg, on_dev)
        if not plans_on:
            got = target.walk_distances(arg, device=on_dev)
            eq('dist', got, dist, where)
        else:
            got = target.walk_plans(arg, it, steps, device=on_dev) if kind == 'slot_walk' else target.walk_plans(it, steps, envs=arg, device=on_dev)
            for name, e in (('plans', plans), ('length', length), ('dist', dist)):
                g = host(getattr(got, name))
                assert g.dtype == np.int32, "%s: %s is %s" % (where, name, g.dtype)
                eq(name, g, e, where)
            self.log('(walk)', kind, (int((length > steps).sum()), int((length < 0).sum())))
        return ('plans' if plans_on else 'dist') + ('/dev' if on_dev else '/host')

    def walk_go(self, kind, where):
        """The macro-action "go to the nearest X and face it", nothing leaving the device: walk_plans(device=True), then rollout(slots, plans,
        limits=length.clamp(0, steps), children=c, device=True).  A pair whose item no reachable pose faces has limit 0 and a column of -1: it
        executes no step, so its child is the parent's row (ngw_snapshot_rollout_path: limits "0 .. n_steps"; the row "as the last executed step
        leaves it" of a pair that executed none) and its reports are 0."""
        rs, spec, K = self.rs, self.spec, self.K
        s, d, parents, children = self.draw_source(rs, self.walk_rows_max())
        count = len(parents)
        steps, items = int(rs.randint(1, WALK_STEPS + 1)), rs.randint(0, K, count).astype(np.int32)
        skip = self.draw_pad(rs, count, True, kind)
        if None in walk_ids(spec.compile()):
            raise Refused(ValueError)
        rows = rows_of(self.src_rows(s))
        walk_skip = None if skip is None or self.side == 'destination' else skip
        dist, plans, length = self.expect_walk(rows, parents, items, steps, walk_skip)
        limits = np.clip(length, 0, steps).astype(np.int32)
        exp = ref_pairs(spec, rows, parents, 'rollout', self.autoreset, self.horizon, plans=np.ascontiguousarray(plans.T), limits=limits)
        live = slice(None) if skip is None else ~skip
        self.write_children(d, children[live], {k: exp['ends'][k][live] for k in STATE_KEYS})
        exp = blank_pairs(exp, skip)
        p, c = self.padded(skip, parents, children)
        p, c = self.dev(p), self.dev(c)
        if s is None:
            wp = self.v.walk_plans(self.dev(items), steps, envs=p, device=True)
        else:
            wp = self.vsnaps[s].walk_plans(p, self.dev(items), steps, device=True)
        got = self.vsnaps[d].rollout(p, wp.plans, children=c, device=True, limits=wp.length.clip(0, steps), **self.src_kw(s, d))
        for name, e in (('plans', plans), ('length', length), ('dist', dist)):
            eq(name, getattr(wp, name), e, where)
        check_pairs(got, exp, 'rollout', False, where)
        self.log('(walk_go)', kind, (int((length[live] < 0).sum()), int((length[live] > steps).sum())))
        return 'envs' if s is None else 'slots'

    # -------------------------------------------------------------- frontiers
    def raise_full(self, full, where):
        """The call that raises the sticky F_FRONTIER_FULL compares the flags at once - ngw_error_flags "reads and clears" -; both sides go on."""
        got, exp = self.v.error_flags(), self.flags | (F_FRONTIER_FULL if full else 0)
        assert got == exp, "%s: error flags %#x, the model says %#x" % (where, got, exp)

    def frontier_compact(self, kind, where):
        """Frontier.compact of a flag tensor of drawn content, taken as a slice that starts 0 .. 15 bytes into a larger one, against frontier_oracle."""
        rs, A = self.rs, self.A
        s = int(rs.randint(0, 2))
        n, off = int(FLAG_LENGTHS[rs.randint(0, len(FLAG_LENGTHS))]), int(rs.randint(0, 16))
        content, div = ('none', 'all', 'sparse', 'stray')[int(rs.randint(0, 4))], int((1, A, 17)[rs.randint(0, 3)])
        with_map, cap_choice = bool(rs.randint(0, 2)), int(rs.randint(0, 4))
        sparse, stray_at = (rs.randint(0, 17, n) == 0).astype(np.uint8), rs.randint(0, max(n, 1), 6)
        amap = (rs.permutation(-(-n // div) + 3) + 7).astype(np.int32)
        flags = {'none': np.zeros(n, np.uint8), 'all': np.ones(n, np.uint8)}.get(content, sparse)
        if content == 'stray' and n:
            flags[stray_at] = np.array([2, 0x80, 0xFF, 2, 0x80, 0xFF], np.uint8)
        big = np.ones(n + 32, np.uint8)                   # (set bytes on both sides of the slice: a load beyond it counts them)
        big[off:off + n] = flags
        total = int(np.count_nonzero(flags))
        capacity = (max(total - 1, 0), 0, total, total + 70)[cap_choice]
        e_first, e_second, e_count, full = FO.compact(flags, div, amap if with_map else None, capacity)
        fr = self.vsnaps[s].frontier(capacity)
        first, second = fr.compact(self.dev(big)[off:off + n], div, self.dev(amap) if with_map else None)
        eq('first', first, e_first, where)
        eq('second', second, e_second, where)
        eq('count', fr.count_dev, np.array(e_count, np.int32), where)
        assert fr.count() == e_count[0] and fr.total() == e_count[1], where
        self.raise_full(full, where)
        fr.close()
        self.log('(compact)', kind, (n, off, content, div, with_map, cap_choice))
        return content

    def frontier_step(self, kind, where):
        """One iteration of the closed loop of frontier.py on a padded parents list: insert_successor_keys -> fresh_pairs -> alloc -> expand."""
        rs, spec, A, ar, H = self.rs, self.spec, self.A, self.autoreset, self.horizon
        d = int(rs.randint(0, 2))
        if not self.filled[d].any():
            d = 0
        cap = self.caps[d]
        live_slots = np.nonzero(self.filled[d])[0]
        parents = live_slots[rs.randint(0, 1 << 30, int(rs.randint(1, 9))) % len(live_slots)].astype(np.int32)
        count = len(parents)
        fields = int(FIELD_CHOICES[rs.randint(0, len(FIELD_CHOICES))])
        cap_choice, mode, u = int(rs.randint(0, 3)), ('ample', 'short', 'exhausted')[int(rs.randint(0, 3))], int(rs.randint(0, 1 << 30))
        skip = self.draw_pad(rs, count, True, kind)
        if self.S > SUCC_MAX_MAP:
            from gym_novel_gridworlds_amd.snapshot import MapsTooLarge
            raise Refused(MapsTooLarge)
        plist = self.padded(skip, parents)
        gone = np.zeros(count, bool) if skip is None else skip
        ex = SU.Successors(spec, self.snaps[d].rows, parents, ar, H)
        keys = ex.keys(fields).copy()
        keys[gone] = 0
        model = self.table.insert(keys.reshape(-1))
        fresh = model[0].reshape(count, A)
        hits = int(fresh.sum())
        capacity = min(max((max(hits - 1, 1), max(hits, 1), hits + 70)[cap_choice], 1), cap)
        e_first, e_second, e_count, full = FO.compact(fresh, A, plist, capacity)
        taken = e_count[0]
        # the cursor: inside the snapshot, and the slots handed out hold no parent of the call (a condition on the draw, made from the model)
        want = {'ample': taken, 'short': max(taken - 1 - u % 3, 0), 'exhausted': 0}[mode]
        busy = np.zeros(cap + 1, np.int64)
        busy[parents[~gone] + 1] = 1
        run = np.cumsum(busy)
        starts = [c for c in range(cap - want + 1) if run[c + want] == run[c]]
        if not starts:
            want, starts = 0, list(range(cap + 1))
        cursor = starts[u % len(starts)]
        limit = None if want == taken and cursor + want == cap and u % 2 else cursor + want
        e_slots, e_cursor, short = FO.alloc(taken, cursor, cap if limit is None else limit, capacity)
        pos, act = np.nonzero(fresh)
        m = min(e_cursor - cursor, capacity)
        kids = ex.child_rows(pos[:m], act[:m])
        self.write_children(d, e_slots[:m], kids)
        rep = {k: np.zeros(capacity, ex.rep[k].dtype) for k in ('reward', 'done', 'result', 'info')}
        for k in rep:
            rep[k][:m] = ex.rep[k][pos[:m], act[:m]]
        # the calls
        pool, pdev = self.vsnaps[d], self.dev(plist)
        succ, found = pool.insert_successor_keys(self.vtable, pdev, fields, device=True)
        fr = pool.frontier(capacity)
        fr.reset_cursor(cursor)
        p, a = fr.fresh_pairs(found.fresh, pdev)
        c = fr.alloc(limit)
        got = pool.expand(p, a, c, device=True)
        SU.assert_successors(succ, ex, fields, where, True, np.nonzero(gone)[0])
        self.check_found(keys.reshape(-1), model, found, where)
        self.last_fields = fields
        eq('parents', p, e_first, where)
        eq('actions', a, e_second, where)
        eq('slots', c, e_slots, where)
        eq('count', fr.count_dev, np.array(e_count, np.int32), where)
        eq('cursor', fr.cursor, np.array([e_cursor], np.int32), where)
        for k in rep:
            eq(k, got[k], rep[k], where)
        self.raise_full(full or short, where)
        fr.close()
        self.log('(step)', kind, (mode, bool(short), bool(full), hits, m))
        return mode

    # -------------------------------------------------------------- the walk
    def run(self):
        rs, v, o, n, A = self.rs, self.v, self.o, self.n, self.A
        tag, log = self.tag, self.log
        v.lidar_configure(self.lc, fused=self.fused, dtype=self.fmt)
        if self.masks_on:
            v.set_action_masks(True)
        self.vsnaps = [v.snapshot(c) for c in self.caps]
        self.vtable = v.key_table(TABLE_CAPACITY)
        self.book = KT.WhereBook(self.vtable.buckets)
        names = sorted(KINDS)
        p = np.array([KINDS[k] for k in names], np.float64)
        p /= p.sum()
        n_calls = int(rs.randint(8, 16))
        kinds = [names[i] for i in rs.choice(len(names), n_calls, p=p)]
        gk = int(rs.randint(1, 4))
        gacts = rs.randint(0, A, size=(gk, n)).astype(np.int32)
        if not self.both_reset(None):
            log('(case)', 'placement', '')
            v.close()
            return
        self.snaps[0].save(o.st, np.arange(n), np.arange(n))   # every env's first state: slots 0 .. n-1 of snapshot 0 stay readable all case long
        self.filled[0][:n] = True
        self.vsnaps[0].save(envs=np.arange(n), slots=np.arange(n))
        self.graph = (gacts, self.dev(gacts))               # one graph, built early; graph_launch is a call kind
        v.graph_build(v.ptr_of(self.graph[1]), n, gk)
        self.check_all(tag + ' setup')
        try:
            for call, kind in enumerate(kinds):
                where = '%s call %d %s' % (tag, call, kind)
                if kind in READ_ONLY:
                    before = state_dict(o.st)
                try:
                    form = self.call(kind, where)
                except Refused as r:
                    try:
                        self.perform_refused(kind)
                    except r.error:
                        pass
                    else:
                        raise AssertionError('%s: the model predicts %s, the env under test raised nothing' % (where, r.error.__name__))
                    log(kind, 'refused', '')
                    self.check_all(where + ' (refused)')
                    continue
                except AssertionError:
                    raise
                except Exception as ex:                   # a refusal the model did not predict
                    raise AssertionError('%s: %s: %s' % (where, type(ex).__name__, ex))
                if form is None:                          # a reset that could not place its items, on both sides
                    log('(case)', 'placement', kind)
                    break
                log(kind, 'executed', form)
                if self.ofail:                            # an in-step reset could not place its items: the env under test must say so too
                    try:
                        v.get_state(); v._raise_flags()
                    except AssertionError as ex:
                        assert 'Cannot place items' in str(ex), where
                    else:
                        raise AssertionError(where + ': only the oracle failed to place')
                    log('(case)', 'placement', kind)
                    break
                if kind in READ_ONLY:
                    assert all((before[k] == getattr(o.st, k)).all() for k in STATE_KEYS), where + ': the model itself moved'
                self.check_all(where, after_steps_injection=kind == 'state_steps')
            else:
                log('(case)', 'completed', '')
        except AssertionError as ex:
            if 'Cannot place items' not in str(ex) or not self.ofail:
                raise
            log('(case)', 'placement', '')
        v.close()

    def perform_refused(self, kind):
        """The refused call on the env under test, in its simplest form (the refusal does not depend on the arguments)."""
        if kind == 'succ_keys':
            self.v.successor_keys()
        elif kind == 'insert_succ_keys':
            self.v.insert_successor_keys(self.vtable, np.zeros(1, np.int32))
        elif kind == 'frontier_step':
            self.vsnaps[0].insert_successor_keys(self.vtable, np.zeros(1, np.int32))
        elif kind == 'walk_go':                           # (a spec without a Forward, a Left or a Right action: "walk plans need ...")
            self.vsnaps[0].walk_plans(np.zeros(1, np.int32), 0, 1)
        else:
            raise AssertionError('no refusal is documented for ' + kind)


def run_case(rs, cfg, case, make_env, log=None):
    """One whole case: settings and calls drawn from `rs`, performed on make_env(...)'s env and on the model, compared after every call."""
    Case(rs, cfg, case, make_env, log).run()


def chunk_cfgs(chunk, chunks):
    return sorted(T.CFGS)[chunk::chunks]
