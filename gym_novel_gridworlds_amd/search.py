"""Device-side search runs of a Snapshot: whole best-first iterations over one node pool and one valued key table, enqueued from ONE call
with no host wait in between (include/ngw.h ngw_search_*; the kernels are csrc/ngw_search.inc, the driver csrc/ngw_abi_search.cpp).

    table = env.key_table(1 << 20, values=True)
    s = pool.search(table, capacity)                      # costs=None: the step costs, round(STEP_COSTS[code] * scale); or an int32 [A] array
    s.reset_cursor(n_roots)                               # the next free slot of the pool
    s.start(roots)                                        # value 0, tag TAG_ROOT; s.g / s.bucket of the roots; s.parents = the roots
    while True:
        s.run(8)                                          # eight iterations, enqueued; returns at once
        goal = s.goal()                                   # the host's poll: the cheapest goal reached so far, (VALUE_NONE, -1) while none is
        if goal.bucket >= 0: break
    t = s.goal_plan(64)                                   # table.trace of the goal's bucket: Trace(plans, length, root)

One iteration is exactly the loop of key_table.py's docstring - successor_keys, insert_min, compact (or select with keep=k), alloc, expand,
called as that loop calls them - with the torch operations between them as three kernels: the OFFER (g[parent] + cost and the tag of every
(parent, action)), the JUDGE (the cheapest goal among the improved positions; with stop_at_goals, ended states are not expanded) and the
SETTLE (the expand lists, g and bucket of the children, the next parents).  relax_reference() states the three in numpy.

That is a LAYERED search (keep=None: every improved child is a parent of the next iteration) or a BEAM (keep=k: the k cheapest children of
this iteration go on, the rest is dropped for good).  open_list=True is the third discipline, a BEST-FIRST search over an open list: a state
that was reached but not yet expanded stays a candidate of every later iteration, ordered by f = g + h - uniform-cost search with h = 0,
A* with a WalkHeuristic over walk_distances, Go-Explore's "the most promising cell of the whole archive" with an f of the caller's own:

    s = pool.search(table, cap, keep=k, open_list=True, heuristic=WalkHeuristic(w, 'min'), prune=True)
    s.reset_cursor(n); s.start(roots)
    while not s.proven(): s.run(8)
    plan = s.goal_plan(64)

An open-list iteration puts a SELECT over s.f (Frontier.select over the whole pool, the `keep` smallest) and a TAKE (the chosen slots are
closed; with prune, those that cannot beat the goal are dropped) in front of the loop above, always compacts, lets the settle SUPERSEDE the
dearer copy of a state reached again, and OPENs the children behind the expand (h from a walk, f = g + h).  take_reference(),
supersede_reference(), open_reference() and best_first_reference() state it in numpy; include/ngw.h is the contract.

A search is rank-local, as a frontier is: under ShardedVecNovelGridworld it belongs to the local env's pool and table."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .frontier import MAX_CAPACITY, MAX_FLAGS, alloc_reference, check_capacity, compact_reference, select_reference
from .key_table import TAG_ROOT, VALUE_NONE, insert_min_reference
from .spec import IDX_NONE, STEP_COSTS

INT32_MIN = -(1 << 31)
MSG_DIED = 14                 # the message code of a FireWall death (Expansion.died)
STATS_ROWS = _cabi.SEARCH_ROWS    # include/ngw.h NGW_SEARCH_ROWS: the iterations stats() keeps

SearchGoal = collections.namedtuple('SearchGoal', 'value bucket')
SearchStats = collections.namedtuple('SearchStats', 'iterations offered improved expanded overflow overflowed cursor flags')
OpenStats = collections.namedtuple('OpenStats', 'iterations chosen pruned superseded open f_min f_bound')
BestFirst = collections.namedtuple('BestFirst', 'chosen parents pruned open f_min f_bound superseded relaxed')
Relaxed = collections.namedtuple('Relaxed', 'values tags best goal parents actions children next_parents cursor offered improved expanded overflow full')


def cost_table(costs, scale, n_actions):
    """The 64 int32 the offer kernel reads and how it indexes them -> (table, by_action).  costs None: round(STEP_COSTS[code] * scale) by the
    cost code of the step's info word - the table of key_table.step_cost_values, refused as there; else `costs`, one int32 per action."""
    lut = np.zeros(64, np.int32)
    if costs is None:
        values = [int(round(c * scale)) for c in STEP_COSTS]
        if not all(0 <= v < VALUE_NONE for v in values):
            raise ValueError("scale: %r takes a step cost outside [0, 2^31 - 1)" % (scale,))
        lut[:len(values)] = values
        return lut, False
    if hasattr(costs, 'data_ptr'):
        costs = costs.cpu().numpy()
    c = np.asarray(costs)
    if c.dtype.kind not in 'iu' or c.shape != (n_actions,):
        raise ValueError("costs: one integer per action expected, shape [%d], got dtype %s, shape %s" % (n_actions, c.dtype, list(c.shape)))
    if c.size and (int(c.min()) < INT32_MIN or int(c.max()) >= VALUE_NONE):
        raise ValueError("costs: an entry outside [-2^31, 2^31 - 1)")
    lut[:n_actions] = c
    return lut, True


def offer_reference(parents, g, bucket, info, n_actions, lut, by_action):
    """Step 2 in numpy -> (values int32 [P * A], tags int32 [P * A], overflow bool [P * A]).  parents int32 [P]; g, bucket int32 [pool]; info
    uint32 [P * A].  Position q = j * A + a offers g[parents[j]] + cost, tagged bucket[parents[j]] * A + a; no offer - (VALUE_NONE, TAG_ROOT) -
    for a parent outside [0, pool) (IDX_NONE is), a g of VALUE_NONE, and a sum outside [-2^31, VALUE_NONE): the last is `overflow`."""
    parents, g, bucket = np.asarray(parents, np.int64), np.asarray(g, np.int64), np.asarray(bucket, np.int64)
    A, P = int(n_actions), len(parents)
    info = np.asarray(info).reshape(-1).astype(np.int64)
    a = np.tile(np.arange(A), P)
    p = np.repeat(parents, A)
    live = (p >= 0) & (p < len(g))
    at = np.where(live, p, 0)
    live &= g[at] != VALUE_NONE
    cost = np.asarray(lut, np.int64)[a if by_action else (info >> 2) & 63]
    total = g[at] + cost
    overflow = live & ((total >= VALUE_NONE) | (total < INT32_MIN))
    live &= ~overflow
    values = np.where(live, total, VALUE_NONE).astype(np.int32)
    tags = np.where(live, bucket[at] * A + a, TAG_ROOT).astype(np.int32)
    return values, tags, overflow


def judge_reference(best, info, values, where, goal=SearchGoal(VALUE_NONE, -1), stop_at_goals=False):
    """Step 4 in numpy -> (best afterwards bool [n], the goal afterwards, improved: the positions with best set).  A position with best set
    whose info word has the done bit (bit 1) and a message code other than 14 is a goal: the smallest (value, bucket) pair of them and of
    `goal` stays.  stop_at_goals: best is cleared wherever the done bit is set."""
    best = np.asarray(best).reshape(-1).astype(bool)
    info = np.asarray(info).reshape(-1).astype(np.int64)
    ended = ((info >> 1) & 1) != 0
    is_goal = best & ended & (((info >> 8) & 255) != MSG_DIED)
    pair = (int(goal[0]), int(goal[1]) & 0xFFFFFFFF)                           # (the bucket ordered as the device orders it: unsigned)
    for q in np.flatnonzero(is_goal).tolist():
        pair = min(pair, (int(values[q]), int(where[q]) & 0xFFFFFFFF))
    bucket = pair[1] - (1 << 32) if pair[1] >= 1 << 31 else pair[1]
    return (best & ~ended if stop_at_goals else best), SearchGoal(pair[0], bucket), int(best.sum())


def settle_reference(first, second, slots, parents, values, where, g, bucket, n_actions):
    """Step 6 in numpy -> (expand's parents int32 [capacity], the next parent list int32 [capacity], expanded).  Entry k of the chosen (first[k]
    = j, second[k] = a) with slot c = slots[k]: the expand pair is (parents[j], a, c); where c is a slot of the pool, g[c] = values[j * A + a],
    bucket[c] = where[j * A + a] (both updated in place) and the next list holds c.  A padded entry gives IDX_NONE in both lists."""
    A, cap = int(n_actions), len(first)
    plist, nxt, expanded = np.full(cap, IDX_NONE, np.int32), np.full(cap, IDX_NONE, np.int32), 0
    for k in range(cap):
        j, a, c = int(first[k]), int(second[k]), int(slots[k])
        if not (0 <= j < cap and 0 <= a < A):
            continue
        plist[k] = parents[j]
        if 0 <= c < len(g):
            g[c], bucket[c], nxt[k] = values[j * A + a], where[j * A + a], c
            expanded += 1
    return plist, nxt, expanded


def relax_reference(parents, g, bucket, info, keys, where, held, cursor, n_actions, lut, by_action, keep=None, stop_at_goals=False,
                    goal=SearchGoal(VALUE_NONE, -1), limit=None):
    """One iteration of Search.run between its successor keys and its expand, in numpy: steps 2 to 6 of include/ngw.h's ngw_search_run ->
    Relaxed.  parents int32 [capacity]; g, bucket int32 [pool], updated in place; info, keys [capacity * A]: what successor_keys reports for
    the parents; where int32 [capacity * A]: the bucket the table gives each key (-1: key 0 or refused - which bucket a key gets is the
    table's choice, so it is an input here); held: the table before the call as insert_min_reference takes it, updated in place; cursor: the
    slot cursor; limit: one past the last slot (None: the pool's size).
    Relaxed.parents / .actions / .children are expand's three lists, .next_parents the frontier of the next iteration, .full whether
    F_FRONTIER_FULL is due (more chosen than `capacity`, or fewer slots left than chosen)."""
    parents = np.asarray(parents, np.int32)
    cap, A = len(parents), int(n_actions)
    where = np.asarray(where, np.int32).reshape(-1)
    ks = np.asarray(keys).reshape(-1)
    ks = ks.astype(np.int64 if ks.dtype.kind == 'i' else np.uint64).view(np.uint64)
    values, tags, overflow = offer_reference(parents, g, bucket, info, A, lut, by_action)
    _, _, best = insert_min_reference(held, ks, values, tags, refused=(where < 0) & (ks != 0))
    best, goal, improved = judge_reference(best, info, values, where, goal, stop_at_goals)
    if keep is None:
        first, second, count, full = compact_reference(best, A, None, cap)
    else:
        first, second, _, _, count = select_reference(values, int(keep), A, None, best, 1, False, cap)
        full = False
    slots, cursor, short = alloc_reference(int(count[0]), cursor, len(g) if limit is None else limit, cap)
    plist, nxt, expanded = settle_reference(first, second, slots, parents, values, where, g, bucket, A)
    return Relaxed(values, tags, best, goal, plist, second, slots, nxt, cursor, int((values != VALUE_NONE).sum()), improved, expanded,
                   int(overflow.sum()), bool(full or short))


class WalkHeuristic(collections.namedtuple('WalkHeuristic', 'weights mode')):
    """The heuristic of an open-list search from walk_distances(): `weights` one int32 >= 0 per item id ([K], K as walk_distances returns),
    `mode` 'min' or 'max'.  With d = walk_distances(slot), h(slot) is the minimum ('min': "walk to the nearest of these") or the maximum
    ('max': "I need all of these") of weights[k] * d[k] over the k with weights[k] > 0 and d[k] >= 0, 0 where there is none; the product is
    taken in 64 bits and clamped to VALUE_NONE - 1 (walk_heuristic_reference).  Whether h is admissible - never above the true cost to a
    goal - is the caller's business.  Rule of thumb: a walk of d moves costs at least d times the cheapest of the spec's three movement costs
    (Forward, Left, Right) under the search's `scale`, so that cost is the weight of an item the goal cannot be reached without facing."""
    __slots__ = ()


H_MODES = {'min': _cabi.SEARCH_H_MIN, 'max': _cabi.SEARCH_H_MAX}


def check_heuristic(heuristic, n_items):
    """-> (mode code, weights int32 [K] or None); ValueError for a bad mode, a wrong shape or dtype, a negative weight."""
    if heuristic is None:
        return _cabi.SEARCH_H_NONE, None
    if not isinstance(heuristic, tuple) or len(heuristic) != 2:
        raise ValueError("heuristic: None or a WalkHeuristic(weights, mode) expected, got %r" % (heuristic,))
    weights, mode = heuristic
    if mode not in H_MODES:
        raise ValueError("heuristic mode: 'min' or 'max' expected, got %r" % (mode,))
    if hasattr(weights, 'data_ptr'):
        weights = weights.cpu().numpy()
    w = np.asarray(weights)
    if w.dtype.kind not in 'iu' or w.shape != (n_items,):
        raise ValueError("heuristic weights: one integer per item id expected, shape [%d], got dtype %s, shape %s" % (n_items, w.dtype, list(w.shape)))
    if w.size and (int(w.min()) < 0 or int(w.max()) > VALUE_NONE):
        raise ValueError("heuristic weights: an entry outside [0, 2^31 - 1]")
    return H_MODES[mode], np.ascontiguousarray(w, np.int32)


def walk_heuristic_reference(dist, weights, mode):
    """h of every row of `dist` (int32 [n, K] or [K], walk_distances' layout) -> int32 [n] (or a scalar array): the minimum ('min') or
    maximum ('max') of int64(weights[k]) * dist[.., k] over the k with weights[k] > 0 and dist[.., k] >= 0, clamped to VALUE_NONE - 1; 0
    where no such k exists."""
    if mode not in H_MODES:
        raise ValueError("heuristic mode: 'min' or 'max' expected, got %r" % (mode,))
    d, w = np.asarray(dist, np.int64), np.asarray(weights, np.int64)
    live = (w > 0) & (d >= 0)
    prod = w * d
    if mode == 'min':
        out = np.where(live, prod, np.iinfo(np.int64).max).min(axis=-1, initial=np.iinfo(np.int64).max)
    else:
        out = np.where(live, prod, -1).max(axis=-1, initial=-1)
    out = np.where(live.any(axis=-1), out, 0)
    return np.minimum(out, VALUE_NONE - 1).astype(np.int32)


def priority_reference(g, h):
    """f = min(int64(g) + h, VALUE_NONE - 1)."""
    return np.minimum(np.asarray(g, np.int64) + np.asarray(h, np.int64), VALUE_NONE - 1).astype(np.int32)


def take_reference(f, keep, capacity, goal_value=VALUE_NONE, prune=False):
    """Step 0 in numpy -> (chosen, parents, pruned, open, f_min, f_bound).  f int32 [pool], updated in place.  The candidates are the slots
    with f != VALUE_NONE (`open`: how many); the `keep` smallest (f, slot) of them are `chosen` (int32 [capacity], ascending slot order,
    IDX_NONE-padded) and closed: f = VALUE_NONE.  `parents` is `chosen` with IDX_NONE where prune is set and the old f is >= goal_value
    (`pruned`: how many); f_min / f_bound: the smallest / largest old f chosen, VALUE_NONE for an empty choice."""
    first, _, taken, _, count = select_reference(f, int(keep), 1, None, None, 1, False, capacity)
    chosen = np.asarray(first, np.int32).copy()
    parents = chosen.copy()
    live = chosen[:int(taken[0])]
    old = np.asarray(f)[live].astype(np.int64)
    f[live] = VALUE_NONE
    cut = old >= int(goal_value) if prune else np.zeros(len(old), bool)
    parents[:len(live)][cut] = IDX_NONE
    return chosen, parents, int(cut.sum()), int(count[1]), int(old.min()) if len(old) else VALUE_NONE, int(old.max()) if len(old) else VALUE_NONE


def supersede_reference(children, bucket, slot_of_bucket, f):
    """The superseding of step 6 in numpy -> how many slots were superseded.  For every child c of `children` (IDX_NONE skipped) with bucket b
    = bucket[c] >= 0: an earlier slot named by slot_of_bucket[b] gets f = VALUE_NONE and is counted; then slot_of_bucket[b] = c.  f and
    slot_of_bucket are updated in place.  (A bucket has at most one child per iteration, so the order of the loop does not matter.)"""
    count = 0
    for c in np.asarray(children).tolist():
        if c == IDX_NONE:
            continue
        b = int(bucket[c])
        if not 0 <= b < len(slot_of_bucket):
            continue
        old = int(slot_of_bucket[b])
        if old >= 0 and old != c:
            f[old] = VALUE_NONE
            count += 1
        slot_of_bucket[b] = c
    return count


def open_reference(children, g, f, h, dist=None, heuristic=None):
    """Step 8 in numpy: for every child c of `children` (IDX_NONE skipped; entry k) h[c] = walk_heuristic_reference(dist[k], ...) - 0 without a
    heuristic - and f[c] = min(int64(g[c]) + h[c], VALUE_NONE - 1); f and h are updated in place.  dist int32 [len(children), K]: the walk
    distances of the children (a padded entry's row is not read)."""
    children = np.asarray(children, np.int64)
    at = np.flatnonzero(children != IDX_NONE)
    c = children[at]
    h[c] = 0 if heuristic is None else walk_heuristic_reference(np.asarray(dist)[at], heuristic[0], heuristic[1])
    f[c] = priority_reference(np.asarray(g)[c], np.asarray(h)[c])


def best_first_reference(f, h, g, bucket, slot_of_bucket, successors, held, cursor, n_actions, lut, by_action, keep, capacity, stop_at_goals=False,
                         goal=SearchGoal(VALUE_NONE, -1), prune=False, heuristic=None, distances=None, limit=None):
    """One OPEN-LIST iteration of Search.run in numpy: steps 0 to 8 of include/ngw.h's "an open-list iteration" -> BestFirst(chosen, parents,
    pruned, open, f_min, f_bound, superseded, relaxed: the Relaxed of steps 2 to 6).  f, h, g, bucket int32 [pool] and slot_of_bucket int32
    [buckets] are updated in place, `held` as in relax_reference.  successors(parents) -> (info, keys, where): what successor_keys reports for
    the parent list and the bucket the table gives each key; distances(children) -> walk_distances of the child list, int32 [capacity, K]
    (only called with a heuristic).  Step 5 always compacts: the choice was made in step 0."""
    chosen, parents, pruned, n_open, f_min, f_bound = take_reference(f, keep, capacity, goal[0], prune)
    info, keys, where = successors(parents)
    r = relax_reference(parents, g, bucket, info, keys, where, held, cursor, n_actions, lut, by_action, None, stop_at_goals, goal, limit)
    superseded = supersede_reference(r.next_parents, bucket, slot_of_bucket, f)
    open_reference(r.next_parents, g, f, h, None if heuristic is None else distances(r.next_parents), heuristic)
    return BestFirst(chosen, parents, pruned, n_open, f_min, f_bound, superseded, r)


# ------------------------------------------------------------------ the recipe heuristic (include/ngw.h ngw_snapshot_recipe_costs; csrc/ngw_recipe.inc)
RecipeRule = collections.namedtuple('RecipeRule', 'out_item out_qty cost inputs tool_item')     # inputs: ((item, qty), ...) consumed; tool_item -1: none
MAX_RULES, MAX_RULE_INPUTS, MAX_MAP_ITEMS = _cabi.RECIPE_MAX_RULES, _cabi.RECIPE_MAX_INPUTS, _cabi.RECIPE_MAX_MAP_ITEMS


class RecipeProgram(collections.namedtuple('RecipeProgram', 'goal_item rules map_items')):
    """What the recipe kernel evaluates: the goal item, at most 16 RecipeRule in topological order - consumers before producers - and
    `map_items`, a bit mask of the items whose cells on the map count as held (recipe_program() builds one from a spec)."""
    __slots__ = ()

    def struct(self):
        """include/ngw.h ngw_recipe_program."""
        if len(self.rules) > MAX_RULES:
            raise ValueError("recipe program: %d rules (at most %d)" % (len(self.rules), MAX_RULES))
        p = _cabi.RecipeProgram()
        p.goal_item, p.n_rules, p.map_items = int(self.goal_item), len(self.rules), int(self.map_items)
        for r, u in enumerate(self.rules):
            if len(u.inputs) > MAX_RULE_INPUTS:
                raise ValueError("recipe rule %d: %d inputs (at most %d)" % (r, len(u.inputs), MAX_RULE_INPUTS))
            q = p.rules[r]
            q.out_item, q.out_qty, q.cost, q.n_in, q.tool_item = int(u.out_item), int(u.out_qty), int(u.cost), len(u.inputs), int(u.tool_item)
            for i, (item, qty) in enumerate(u.inputs):
                q.in_item[i], q.in_qty[i] = int(item), int(qty)
        return p


def recipe_program(spec, costs=None, scale=1):
    """The relaxed-plan program of a spec (an EnvSpec or a compiled ngw_spec) under a search's cost table - `costs` / `scale` as pool.search
    takes them, through cost_table -> RecipeProgram.  A rule is ONE successful application of one action, at that action's cost
    (round(STEP_COSTS[its success code] * scale), or costs[its action id]):
        craft    a recipe: its inputs are consumed, recipe_out_qty comes out (cost code cost_ok);
        extract  the spec's extract rule: ext_qty of ext_out (cost code ext_cost_ok).  The source is a BLOCK IN FRONT of the agent, never the
                 inventory: where the step consumes it (Bow: a wool block -> 4 string) the rule has no input - what it takes for the block to
                 be there is left out -, where it stays (Pogostick: the tap -> 1 rubber) it is the rule's TOOL;
        break    an item that lies on the map at reset and has no recipe and is not extracted: no input, break_qty[item] come out (cost_break;
                 with an axe in the spec the cheaper of the two costs and the larger of the two quantities).
    An item with more than one source - a recipe and the extract rule, a recipe and the map (the v0 ids' sticks and planks), a crate, a Chop
    action beside Break - gets NO rule, and so does one whose action the spec lacks: demand on it costs 0, the bound is weaker there and never
    wrong.  Only the rules the goal item's demand can reach are kept, consumers before producers (ties: the smaller item id); a recipe table
    with a cycle among them raises ValueError, as do a negative rule cost and more than 16 rules.  map_items flags the tools - at most 4 -
    that no kept rule consumes: a tap standing on the map serves as one in the inventory does (so being on the map is no second source of a
    flagged item).
    What the rules leave out - Place, "the tap must stand beside a tree", the crafting table, every move - only lowers the bound.  Whether it
    is admissible for a spec is the caller's business, as with WalkHeuristic; tests/test_recipe_heuristic_cpu.py shows consistency, which
    gives it, for the base Pogostick-v1 and Bow-v1 specs."""
    from .spec import ACT_BREAK, ACT_CHOP, ACT_CRAFT, ACT_EXTRACT
    cs = spec.compile() if hasattr(spec, 'compile') else spec
    K, A = int(cs.n_items), int(cs.n_actions)
    lut, by_action = cost_table(costs, scale, A)
    kinds, args = [int(cs.act_kind[a]) for a in range(A)], [int(cs.act_arg[a]) for a in range(A)]

    def cost_of(kind, arg, code):
        """The cost of the lowest action id of `kind` (and `arg`), None when the spec has no such action."""
        ids = [a for a in range(A) if kinds[a] == kind and (arg is None or args[a] == arg)]
        if not ids:
            return None
        return int(lut[ids[0]] if by_action else lut[code])

    sources = [[] for _ in range(K)]                     # per item: the rules that give it, or None for a source that is no rule
    for r in range(int(cs.n_recipes)):
        out = int(cs.recipe_out_item[r])
        inputs = tuple((int(cs.recipe_in_item[r][j]), int(cs.recipe_in[r][int(cs.recipe_in_item[r][j])])) for j in range(int(cs.recipe_n_in[r])))
        cost = cost_of(ACT_CRAFT, r, int(cs.cost_ok[r]))
        sources[out].append(None if cost is None else RecipeRule(out, int(cs.recipe_out_qty[r]), cost, inputs, -1))
    if ACT_EXTRACT in kinds and int(cs.ext_qty) > 0:
        out, src = int(cs.ext_out), int(cs.ext_src)
        cost = cost_of(ACT_EXTRACT, None, int(cs.ext_cost_ok))
        sources[out].append(None if cost is None else RecipeRule(out, int(cs.ext_qty), cost, (), -1 if cs.ext_consume else src))
    tools = {u.tool_item for s in sources for u in s if u is not None and u.tool_item >= 0}
    on_map = {int(cs.start_item[j]) for j in range(int(cs.n_start))} | {int(cs.pass_item[j]) for j in range(int(cs.n_passes))}
    if int(cs.tap_item):
        on_map.add(int(cs.tap_item))
    for k in sorted(on_map - tools):                     # (a tool on the map is counted as held: map_items)
        cost, qty = cost_of(ACT_BREAK, None, int(cs.cost_break)), int(cs.break_qty[k])
        if int(cs.axe_item) and not by_action and cost is not None:
            cost, qty = min(cost, int(lut[int(cs.axe_cost)])), max(qty, int(cs.axe_qty))
        ok = cost is not None and cs.breakable[k] and qty >= 1 and ACT_CHOP not in kinds
        sources[k].append(RecipeRule(k, qty, cost, (), -1) if ok else None)
    for k in range(K):
        if cs.crate_add[k]:
            sources[k].append(None)
    rule_of = {k: s[0] for k, s in enumerate(sources) if len(s) == 1 and s[0] is not None}
    goal = int(cs.goal_item)
    reach, stack = set(), [goal]
    while stack:                                         # the rules the goal's demand can reach
        k = stack.pop()
        if k in reach or k not in rule_of:
            continue
        reach.add(k)
        stack += [item for item, _ in rule_of[k].inputs] + ([rule_of[k].tool_item] if rule_of[k].tool_item >= 0 else [])
    feeds = {k: {item for item, _ in rule_of[k].inputs} | ({rule_of[k].tool_item} - {-1}) for k in reach}
    waiting = {k: sum(1 for c in reach if k in feeds[c]) for k in reach}          # consumers not yet emitted
    rules, left = [], set(reach)
    while left:
        ready = sorted(k for k in left if waiting[k] == 0)
        if not ready:
            raise ValueError("recipe table: a cycle among the rules of items %s" % sorted(left))
        k = ready[0]
        left.remove(k)
        rules.append(rule_of[k])
        for item in feeds[k] & reach:
            waiting[item] -= 1
    if len(rules) > MAX_RULES:
        raise ValueError("recipe program: %d rules (at most %d)" % (len(rules), MAX_RULES))
    for u in rules:
        if u.cost < 0:
            raise ValueError("recipe program: the rule of item %d has a negative cost (%d): no lower bound comes of it" % (u.out_item, u.cost))
    consumed = {item for u in rules for item, _ in u.inputs}
    flagged = sorted({u.tool_item for u in rules if u.tool_item >= 0} - consumed)[:MAX_MAP_ITEMS]
    return RecipeProgram(goal, tuple(rules), sum(1 << k for k in flagged))


def map_item_counts(maps, n_items):
    """on_map for recipe_cost_reference: int32 [n, K], how many cells of each map ([n, S * S] or [n, S, S] item ids) hold each id."""
    m = np.asarray(maps)
    m = m.reshape(m.shape[0], -1)
    return np.stack([(m == k).sum(axis=1) for k in range(int(n_items))], axis=1).astype(np.int32)


def recipe_cost_reference(inv, on_map, program):
    """The recipe heuristic in numpy (the contract of include/ngw.h, ngw_snapshot_recipe_costs) -> int32 [n] (a scalar array for one row).
    inv int32 [n, K] or [K]: the inventories; on_map the same shape (map_item_counts of the maps) or None: nothing on any map.
        have[k] = inv[k] + (on_map[k] if bit k of program.map_items is set);  need[goal] = 1, every other need 0;  h = 0
        for each rule in order:  d = max(0, need[out] - have[out]);  n = ceil(d / out_qty);  h += n * cost;  need[in_i] += n * in_qty_i;
                                 if n > 0 and the rule has a tool: need[tool] = max(need[tool], 1)
    in 64 bits, need saturating at 2^31 - 1 and h at VALUE_NONE - 1."""
    inv = np.asarray(inv, np.int64)
    one = inv.ndim == 1
    have = inv.reshape(-1, inv.shape[-1]).copy()
    K = have.shape[1]
    if on_map is not None:
        flagged = np.array([(int(program.map_items) >> k) & 1 for k in range(K)], np.int64)
        have += np.asarray(on_map, np.int64).reshape(have.shape) * flagged
    need = np.zeros_like(have)
    need[:, int(program.goal_item)] = 1
    h = np.zeros(len(have), np.int64)
    for u in program.rules:
        d = np.maximum(need[:, u.out_item] - have[:, u.out_item], 0)
        n = (d + (int(u.out_qty) - 1)) // int(u.out_qty)
        h = np.minimum(h + n * int(u.cost), VALUE_NONE - 1)
        for item, qty in u.inputs:
            need[:, item] = np.minimum(need[:, item] + n * int(qty), (1 << 31) - 1)
        if u.tool_item >= 0:
            need[:, u.tool_item] = np.where(n > 0, np.maximum(need[:, u.tool_item], 1), need[:, u.tool_item])
    h = h.astype(np.int32)
    return h[0] if one else h


class RecipeHeuristic(collections.namedtuple('RecipeHeuristic', 'walk')):
    """The heuristic of an open-list search from the recipe table: h(slot) = min(recipe + walk, VALUE_NONE - 1), `recipe` the relaxed-plan
    cost of the slot's state under recipe_program(the env's spec, the search's own costs / scale) - what the crafts, extractions and breaks
    still cost at the least - and `walk` the term of a WalkHeuristic (None: 0).  Movement actions and rule actions are disjoint, so the sum of
    two lower bounds is one.  Whether it is admissible is the caller's business, as WalkHeuristic says."""
    __slots__ = ()

    def __new__(cls, walk=None):
        return super().__new__(cls, walk)


def recipe_call(env, holder, s, idx, limit, name, costs, scale, device):
    """The one launch behind Snapshot.recipe_costs (s: the C handle of the snapshot the rows are read from) and VecNovelGridworld.recipe_costs
    (s None: the envs' current states): idx indexes rows [0, limit); `holder` keeps an uploaded list alive.  -> int32 [count]."""
    import torch

    from .snapshot import check_slots, enqueue_ordered, tensor_len, upload
    program = recipe_program(env.cspec, costs, scale).struct()
    dev = torch.device('cuda:%d' % env.device)
    rows, count = check_slots(idx, limit, lambda x: tensor_len(dev, name, x), False, name)
    (ptr,), uploaded = upload(dev, count, rows)
    out = torch.empty(count, dtype=torch.int32, device=dev)
    enqueue_ordered(env, holder, lambda: _cabi.lib().ngw_snapshot_recipe_costs(env._h, s, ptr, count, C.byref(program), C.c_void_p(out.data_ptr())), count,
                    uploaded, device)
    return out if device else out.cpu().numpy()


def check_roots(roots, limit, capacity, device_len=None):
    """The host-side check of start()'s roots: a list / numpy array of one dimension and integer dtype whose entries are slots in [0, limit) or
    IDX_NONE -> a contiguous int32 array; device_len(x): the length of x when it is a device tensor to be used in place (its values are then
    not checked), else None.  At most `capacity` roots.  Returns (roots, count)."""
    n = None if device_len is None else device_len(roots)
    if n is None:
        if roots is None:
            raise ValueError("roots: a list of slots expected")
        a = np.asarray(roots)
        if a.size == 0 and a.ndim == 1:
            a = np.zeros(0, np.int32)
        if a.dtype.kind not in 'iu':
            raise ValueError("roots: integer slots expected, got dtype %s" % a.dtype)
        if a.ndim != 1:
            raise ValueError("roots: a one-dimensional list expected, got shape %s" % (a.shape,))
        bad = a[(a != IDX_NONE) & ((a < 0) | (a >= limit))]
        if bad.size:
            raise ValueError("roots: %d outside [0, %d)" % (int(bad[0]), limit))
        roots, n = np.ascontiguousarray(a, np.int32), int(a.size)
    if n > capacity:
        raise ValueError("roots: %d roots in a search of capacity %d" % (n, capacity))
    return roots, int(n)


class Search:
    """Whole best-first iterations over one Snapshot (the node pool) and one KeyTable made with values=True (Snapshot.search).  It owns, in the
    env's device memory, two parent lists that take turns (`parents`: the current one, int32 [capacity], IDX_NONE-padded), `g` and `bucket`
    (int32 [pool.capacity]: the cost and the bucket each slot was reached with, VALUE_NONE / -1 before), `cursor` (int32 [1]: the next slot
    the allocation hands out) and the scratch of capacity * A entries per array; run() allocates nothing.  start() and run() are enqueued on
    the env's stream and return at once; goal() and stats() wait.  The tensors are views of the library's memory: they are gone with close(),
    with the snapshot, the table or the env.
    costs: None - the step costs, round(STEP_COSTS[code] * scale) by each step's cost code (key_table.step_cost_values' table) -, or one
    int32 per action.  keep: None - every state reached more cheaply goes on (Frontier.compact) -, or k: the k cheapest of them
    (Frontier.select, one group, by g alone; ties: the smaller position).  stop_at_goals: a state whose step reported done - goal or
    FireWall death - is stored and valued but never expanded.
    An offer never wraps: where g + cost would reach VALUE_NONE no offer is made, and stats() counts it (step_cost_values on the host wraps
    silently, as it says).  F_FRONTIER_FULL, F_TABLE_FULL and F_BAD_INDEX are raised where the hand-written loop raises them.
    open_list=True (requires 1 <= keep <= capacity): a best-first search over an OPEN LIST.  `keep` is then how many open states an iteration
    expands, chosen from the WHOLE open list by the smallest f (ties: the smaller slot); `capacity` stays the width of the lists, so it bounds
    the children written per iteration - keep * A <= capacity guarantees that no improved child is dropped by the compaction (it is not
    enforced: F_FRONTIER_FULL reports a drop).  Two more tensors, views as g and bucket are: `h` (int32 [pool.capacity]: the heuristic of the
    state in each slot, 0 until written) and `f` (int32 [pool.capacity]: the priority of each OPEN slot; VALUE_NONE for a slot that is
    unreached, closed - expanded, pruned or superseded - or never opened).  The library reads f only in the selection and writes it only
    where an iteration says (closing the chosen and the superseded, opening the children and the roots): a caller who runs run(1) and
    rewrites f of the open slots with a torch expression of their own - a learned value, say - gets that order.  A slot written by anything
    but the search keeps f = VALUE_NONE and is never chosen.  After start() `parents` is empty - the first iteration chooses the roots from
    the list -; after run() it holds the children the last iteration wrote and `chosen` the slots it expanded.
    heuristic: None (h = 0: uniform-cost search), a WalkHeuristic, or a RecipeHeuristic(walk=None | WalkHeuristic) - the crafting-cost lower
    bound of recipe_program(spec, costs, scale) plus the walk term; `recipe` is then that program.  prune=True: a chosen slot whose f is >= the goal's value is closed
    without being expanded - valid for an admissible h and non-negative costs -, so once a goal is known iterations stop expanding what
    cannot beat it, and when nothing can they expand nothing (the launches leave early on empty lists): the early stop on the device."""

    def __init__(self, snap, table, capacity, costs=None, scale=1, keep=None, stop_at_goals=False, open_list=False, heuristic=None, prune=False):
        import torch
        from .snapshot import MapsTooLarge
        from .vec_env import _DevArray
        self.snap, self.env, self.table = snap, snap.env, table
        snap._open()
        if not hasattr(table, '_open_for'):
            raise ValueError("table: a KeyTable expected")
        table._open_for(self.env)
        table._valued()
        self.capacity = check_capacity(capacity)
        A = self.env.n_actions
        if not 1 <= self.capacity <= snap.capacity:
            raise ValueError("capacity: %d outside [1, the pool's %d]" % (self.capacity, snap.capacity))
        if self.capacity * A > MAX_FLAGS:
            raise ValueError("capacity: %d parents by %d actions in one iteration (at most 2^24 positions)" % (self.capacity, A))
        if keep is not None:
            if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or not 0 <= keep <= MAX_CAPACITY:
                raise ValueError("keep: None or an integer in [0, 2^31 - 1] expected, got %r" % (keep,))
            if keep > self.capacity:
                raise ValueError("keep: %d entries do not fit the capacity %d" % (keep, self.capacity))
        self.keep, self.stop_at_goals = (None if keep is None else int(keep)), bool(stop_at_goals)
        self.open_list, self.prune, self.heuristic = bool(open_list), bool(prune), heuristic
        if not self.open_list and (heuristic is not None or prune):
            raise ValueError("heuristic / prune: only an open-list search has them (open_list=True)")
        if self.open_list:
            if self.keep is None or self.keep < 1:
                raise ValueError("keep: an open-list search expands 1 <= keep <= capacity states per iteration, got %r" % (keep,))
            if snap.capacity > MAX_FLAGS:
                raise ValueError("open_list: the selection runs over every slot of the pool, at most 2^24 (this pool has %d)" % snap.capacity)
        walk = heuristic.walk if isinstance(heuristic, RecipeHeuristic) else heuristic
        mode, weights = check_heuristic(walk, self.env.n_items)
        self.costs, self.by_action = cost_table(costs, scale, A)
        self.recipe = recipe_program(self.env.cspec, costs, scale) if isinstance(heuristic, RecipeHeuristic) else None
        self._s, self._keep, self._cur = C.c_void_p(), None, 0
        more = _cabi.SearchArraysOpen()
        arrays = more.base
        try:
            if self.open_list:
                opt = _cabi.SearchOptions(self.capacity, _cabi._ptr(self.costs, np.int32), int(self.by_action), self.keep, int(self.stop_at_goals), int(self.prune),
                                          mode, 0 if weights is None else len(weights), _cabi._ptr(weights, np.int32))
                _cabi.check(_cabi.lib().ngw_search_create_open(self.env._h, snap._s, table._t, C.byref(opt), C.byref(more), C.byref(self._s)))
            else:
                _cabi.check(_cabi.lib().ngw_search_create(self.env._h, snap._s, table._t, self.capacity, _cabi._ptr(self.costs, np.int32), int(self.by_action),
                                                          -1 if self.keep is None else self.keep, int(self.stop_at_goals), C.byref(arrays), C.byref(self._s)))
        except ValueError as e:
            if str(e).startswith('map_size'):
                raise MapsTooLarge(str(e)) from None
            raise
        if self.recipe is not None:                     # (before any start: the term's scratch is allocated here, run() allocates nothing)
            try:
                _cabi.check(_cabi.lib().ngw_search_set_recipe(self.env._h, self._s, C.byref(self.recipe.struct())))
            except Exception:
                _cabi.lib().ngw_search_destroy(self.env._h, self._s)
                self._s = C.c_void_p()
                raise
        dev = 'cuda:%d' % self.env.device
        view = lambda ptr, n: torch.as_tensor(_DevArray(ptr, (n,), '<i4'), device=dev)   # noqa: E731
        self._lists = [view(arrays.parents[0], self.capacity), view(arrays.parents[1], self.capacity)]
        self.g, self.bucket, self.cursor = view(arrays.g, snap.capacity), view(arrays.bucket, snap.capacity), view(arrays.cursor, 1)
        self.h, self.f = (view(more.h, snap.capacity), view(more.f, snap.capacity)) if self.open_list else (None, None)
        self._dev = torch.device(dev)

    def _open(self):
        if not self._s:
            raise ValueError("search is closed")
        self.snap._open()
        self.table._open_for(self.env)
        return self._s

    @property
    def parents(self):
        """The current frontier: int32 [capacity], IDX_NONE-padded (the list the next iteration expands)."""
        self._open()
        return self._lists[self._cur]

    @property
    def chosen(self):
        """An open-list search: the slots the last iteration expanded - int32 [capacity], ascending, IDX_NONE where pruned and behind them
        (the other of the two parent lists: step 0's choice after the take; all IDX_NONE before the first iteration)."""
        self._open()
        if not self.open_list:
            raise ValueError("chosen: only an open-list search has it (open_list=True)")
        return self._lists[self._cur ^ 1]

    def _enqueue(self, call, uploaded=()):
        from .snapshot import enqueue_ordered
        cur = C.c_int32(self._cur)
        try:
            enqueue_ordered(self.env, self, lambda: call(C.byref(cur)), 1, list(uploaded), True)
        finally:
            self._cur = int(cur.value)
        # An uploaded list need not be held for the next call to synchronise on: it was allocated on torch's current stream, which
        # enqueue_ordered has just made wait for the env's stream, and torch's allocator hands a freed block only to later work of the
        # stream it was allocated on - work that is ordered behind the launch that reads the list.  So start(list); run(k) has no host wait.
        self._keep = None

    def reset_cursor(self, start=0):
        """The next slot the allocation hands out (on torch's current stream; no host wait) - as on Frontier."""
        self._open()
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start <= MAX_CAPACITY:
            raise ValueError("start: an integer in [0, 2^31 - 1] expected, got %r" % (start,))
        self.cursor.fill_(int(start))

    def start(self, roots):
        """The roots of the search - slots of the pool: a list / numpy array (checked; IDX_NONE is allowed and skipped) or a contiguous torch
        int32 tensor on the env's device, used in place; at most `capacity`.  Their keys are offered to the table with value 0 and tag
        TAG_ROOT (insert_keys_min); g[root] = the value the table then holds, bucket[root] = its bucket, and `parents` becomes the roots -
        IDX_NONE where a root's state was already held at a value of 0 or below, as the second position of a repeated state is.  An
        open-list search opens those roots instead - h[root], f[root] = min(g + h, VALUE_NONE - 1) - and leaves `parents` empty; a second
        start() adds its roots to the open list that is there (f, h and the superseding's slots stay), so after table.clear() make a new
        search instead of restarting this one.  Enqueued; no host wait."""
        from .snapshot import tensor_len, upload
        s = self._open()
        r, count = check_roots(roots, self.snap.capacity, self.capacity, lambda x: tensor_len(self._dev, 'roots', x))
        (ptr,), uploaded = upload(self._dev, count, r)
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda cur: L.ngw_search_start(h, s, ptr, count, cur), uploaded)

    def run(self, iterations=1):
        """`iterations` whole iterations, enqueued on the env's stream; returns at once.  An iteration whose frontier is empty runs the same
        launches, which leave early."""
        s = self._open()
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= MAX_CAPACITY:
            raise ValueError("iterations: an integer in [0, 2^31 - 1] expected, got %r" % (iterations,))
        h, L = self.env._h, _cabi.lib()
        self._enqueue(lambda cur: L.ngw_search_run(h, s, int(iterations), cur))

    def _read(self):
        rep = _cabi.SearchReport()
        _cabi.check(_cabi.lib().ngw_search_read(self.env._h, self._open(), C.byref(rep)))
        return rep

    def goal(self):
        """SearchGoal(value, bucket): the cheapest goal the search has reached - the smallest (value, bucket) among the positions that
        brought a goal state a smaller value -, (VALUE_NONE, -1) while none was.  Waits for the env's stream."""
        rep = self._read()
        return SearchGoal(int(rep.goal_value), int(rep.goal_bucket))

    def goal_plan(self, steps, device=False):
        """table.trace of the goal's bucket: Trace(plans [steps, 1], length [1], root [1]) - the cheapest plan found to the goal, from its
        root; length -1 while no goal was reached.  Waits (goal())."""
        return self.table.trace(np.array([self.goal().bucket], np.int32), steps, device=device)

    def stats(self):
        """SearchStats: iterations run; offered / improved / expanded / overflow, uint32 arrays with one entry per iteration of the last 64,
        oldest first - the positions that made an offer, those that brought their key a smaller value, the children written, the offers
        dropped because g + cost left the int32 range -; overflowed: the last over the whole search; cursor: the next free slot; flags: the
        env's sticky flags (error_flags()), left standing.  Waits for the env's stream."""
        rep = self._read()
        rows = np.ctypeslib.as_array(rep.stats).reshape(STATS_ROWS, 4)[:rep.rows].copy()
        return SearchStats(int(rep.iterations), rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], int(rep.overflowed), int(rep.cursor), int(rep.flags))

    def open_stats(self):
        """An open-list search: OpenStats - iterations run; chosen / pruned / superseded / open / f_min / f_bound, int32 arrays with one entry
        per iteration of the last 64, oldest first: the slots the selection took, those of them pruned, the earlier copies superseded, the
        candidates in the list before the choice, and the smallest and largest f chosen (VALUE_NONE for an empty choice).  sum(chosen -
        pruned) is the number of states expanded.  Waits for the env's stream, as stats() does."""
        s = self._open()
        if not self.open_list:
            raise ValueError("open_stats: only an open-list search has them (open_list=True)")
        rep = _cabi.SearchOpenReport()
        _cabi.check(_cabi.lib().ngw_search_read_open(self.env._h, s, C.byref(rep)))
        rows = np.ctypeslib.as_array(rep.stats).reshape(STATS_ROWS, 6)[:rep.rows].copy()
        return OpenStats(int(rep.iterations), *(rows[:, i] for i in range(6)))

    def proven(self):
        """An open-list search: True when a goal is known and the last iteration run reported open == 0 or f_min >= goal().value.  For an
        admissible h that proves the goal cheapest: f_min is the minimum of the whole open list at the start of that iteration, every
        cheapest path has a state on the list whose f is at most the cheapest cost C*, so C* >= f_min >= goal.value >= C* - provided no
        state was lost, which means no F_FRONTIER_FULL and no F_TABLE_FULL (stats().flags).  Waits, as goal() does."""
        st = self.open_stats()
        goal = self.goal()
        if goal.value == VALUE_NONE or not len(st.open):
            return False
        return bool(st.open[-1] == 0 or st.f_min[-1] >= goal.value)

    @property
    def closed(self):
        return not self._s

    def close(self):
        if self._s and self.env._h:
            _cabi.check(_cabi.lib().ngw_search_destroy(self.env._h, self._s))
        self._invalidate()
        searches = self.snap.__dict__.get('_searches')
        if searches and self in searches:
            searches.remove(self)

    def _invalidate(self):
        """The handle is gone (or going), and the arrays with it."""
        self._s = C.c_void_p()
        self._lists = self.g = self.bucket = self.cursor = self.h = self.f = None
        self._keep = None
